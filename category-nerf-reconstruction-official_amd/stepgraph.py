"""Everything between "n steps are wanted" and "these hipGraphs were launched", once, for the category trainer, the background
step and the whole iteration (fused.FusedCategoryTrainer, background.BackgroundStep, background.FullStepTrainer).

A step owner is a BRANCH.  The driver asks four things of it and touches nothing else:

    before_step()       host work due before the next step (the reshuffle at an epoch end, the background's repack); returns the
                        steps left before the next host-launched epoch end
    record(slot, par)   one step's launches on the current stream, reading state parity ``par``; ``slot``: the history slot a step
                        that is not the last of its launch leaves its loss values in, or None
    advance(U)          host bookkeeping after a launch of U steps (cursor, steps_done, parity, ...)
    parity, steps_done  the capture-time state a graph depends on (always 0 for the background), the steps run so far

Graph keys: ``parity`` for one step, ``(parity, U)`` for a group of U.  A group is even, so it leaves the parameter / state
ping-pong where it found it, and it never crosses an epoch end of any branch: the reshuffles are host-launched."""
import contextlib
import gc
import threading

import torch

_CAPTURE_LOCK = threading.Lock()


def group_sizes(U0):
    """group sizes of the multi-step graphs, largest first: EVERY even size U0, U0 - 2, .., 2.  (A halving ladder -- U0,
    U0 / 2, .. -- sent the 7 steps in front of an epoch end and the 13 behind it out as 4 + 2 + 1 and 10 + 2 + 1: six graph
    launches and the reshuffle's three kernels in a row, ~400 us of host work against ~400 us of GPU work queued: a 20-step
    region with an epoch end inside ran 82 us per step.  With every even size it is 6 + 1 and 12 + 1.)"""
    return list(range(int(U0) // 2 * 2, 1, -2))


def plan_group(n, left, unroll, graphs):
    """Which launch goes out next: U, the largest even group that fits the ``n`` steps still wanted, the ``left`` steps before
    the next epoch end (the minimum over the branches) and ``unroll`` -- each launch boundary idles the GPU ~8 us -- or 0 for a
    single step.  ``graphs``: warm-up is over and groups are allowed.  (``group_sizes`` holds every even size, so the largest of
    them that fits is the smallest of the three bounds rounded down to even: no list, no loop in front of every launch.)"""
    return min(n, left, unroll) // 2 * 2 if graphs else 0


class StepGraphs:
    """``branches``: one, or the main one and the one that may run beside it.  ``warmup``: eager steps before anything is
    captured (the first steps allocate the buffers a graph holds on to).  ``unroll``: the largest group (the main branch has
    unroll - 1 history slots).  ``layout`` of two branches in a graph -- they share no parameter and no buffer --:

      "free"    one fork at the top, the side branch's U bodies on the side stream, the main one's on the capturing stream, one
                join at the end: iteration i + 1 of one chain waits for nothing of the other
      "iter"    fork and join in every iteration
      "single"  one stream, the side branch's step in front of the main one's

    ``groups=False``: single steps only.  ``single(graph)``: launches one step in place of record / capture (the category
    trainer's two graphs around a gradient all-reduce)."""

    def __init__(self, branches, warmup, unroll=2, layout="single", side=None, groups=True, single=None):
        self.main, self.side = branches[0], (branches[1] if len(branches) > 1 else None)
        self.warmup, self.unroll, self.layout = warmup, unroll, layout
        self._stream, self.groups, self.single = side, groups, single
        self.graphs, self.steps_done = {}, 0           # (steps_done: steps sent out by this driver)
        self._warm = False

    # ---- the three touch points of the device (a host test replaces them with recorders) ----------------------------------------
    def capture(self, fn, pool=None):
        """record (not run) what ``fn`` launches; returns the object whose ``replay()`` runs it.  A step owner and its driver
        refer to each other, so a discarded owner -- its graphs and their memory pool with it -- lives until the cycle collector
        finds it.  If that happens inside a capture, the graphs are destroyed and their memory freed under a capturing
        stream, which the runtime does not allow (the process aborts).  Older torch collected in front of every capture; torch 2.10 does
        so only with torch.compiler.config.force_cudagraph_gc: collect here, and hold the collector off until the capture ends."""
        g = torch.cuda.CUDAGraph()
        with _CAPTURE_LOCK:                            # gc.disable() is process-wide: one capture at a time owns the switch
            gc.collect()
            enabled = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g, pool=pool):
                    fn()
            finally:
                if enabled:
                    gc.enable()
        return g

    def fork(self):
        """the side stream, made to wait for the current one: a context"""
        self._stream.wait_stream(torch.cuda.current_stream())
        return torch.cuda.stream(self._stream)

    def join(self):
        torch.cuda.current_stream().wait_stream(self._stream)

    # ---- recording and launching -------------------------------------------------------------------------------------------
    def record(self, par, U):
        """the launches of U steps from state parity ``par`` on the current stream (and the side stream), in ``layout``"""
        steps = [(i if i < U - 1 else None, par ^ (i & 1)) for i in range(U)]
        two = self.side is not None and self.layout != "single"
        for chunk in ([steps] if self.layout == "free" else [[s] for s in steps]):
            if self.side is not None:
                with (self.fork() if two else contextlib.nullcontext()):
                    for s in chunk:
                        self.side.record(*s)
            for s in chunk:
                self.main.record(*s)
            if two:
                self.join()

    def _graph(self, par, U):
        key = par if U == 1 else (par, U)
        if key not in self.graphs:
            self.graphs[key] = self.capture(lambda: self.record(par, U))
        return self.graphs[key]

    def _ready(self, graph):
        """graphs are wanted and every branch has run its warm-up steps (wherever: a branch stepped on its own has its buffers)"""
        if not self._warm:
            self._warm = min(b.steps_done for b in (self.main, self.side) if b is not None) >= self.warmup
        return self._warm and bool(graph)

    def step(self, graph=True):
        """one step of every branch: eager during warm-up or with ``graph`` false, else one replay"""
        self.run(1, graph=graph)

    def run(self, n, unroll=None, graph=True):
        """``n`` steps, the same launches as ``n`` calls of ``step()``, in as few graph launches as the epoch ends allow.  (The
        loop body runs in front of a GPU that may be idle: few calls, no inner loop, no allocation.)"""
        unroll = min(self.unroll if unroll is None else max(2, int(unroll)), self.unroll)
        main, side, graphs = self.main, self.side, self.graphs
        while n > 0:
            left = main.before_step()
            if side is not None:
                left = min(left, side.before_step())
            ready = self._warm and graph or self._ready(graph)
            U = plan_group(n, left, unroll, ready and self.groups) or 1
            par = main.parity
            if U == 1 and self.single is not None:
                self.single(ready)
            elif ready:
                (graphs.get(par if U == 1 else (par, U)) or self._graph(par, U)).replay()
            else:
                self.record(par, 1)
            main.advance(U)
            if side is not None:
                side.advance(U)
            self.steps_done += U
            n -= U

    def prepare(self, unroll=None, graph=True):
        """Capture every graph ``step()`` / ``run()`` can need -- one step and every group up to ``unroll``, from either state
        parity -- without running them, so that no capture (a millisecond of host work) lands inside a timed or latency-sensitive
        region later.  A no-op without graphs, without groups and during warm-up (the buffers do not exist yet)."""
        if not (self._ready(graph) and self.groups):
            return
        unroll = min(self.unroll if unroll is None else max(2, int(unroll)), self.unroll)
        for par in (0, 1):
            for U in (1, *group_sizes(unroll)):
                self._graph(par, U)
