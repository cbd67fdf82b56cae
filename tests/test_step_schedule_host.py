"""CPU: the one scheduler of step graphs (stepgraph.StepGraphs: which launches go out for "n steps", what a graph records, what
the branches book afterwards) driven with fake branches and recording capture / fork / join methods -- no GPU, no kernel library.

The expected launch sequences are a line-by-line restatement of the loops the scheduler replaced (FusedCategoryTrainer.run /
.step and FullStepTrainer.run / .step before it).  Notation: ``e`` an eager step, ``g1@p`` the single-step graph of parity p,
``U@p`` a group of U steps from parity p, ``S`` a reshuffle (``So`` / ``Sb``: of the category / background branch), ``|``
between two run() calls."""
import contextlib

import pytest


@pytest.fixture(scope="module")
def sg():
    import cnr_amd
    return cnr_amd.stepgraph


class FakeBranch:
    """a pool length, rays per step, a cursor and a parity (which only the category branch flips)"""

    def __init__(self, name, slices, rays, log, flips=True):
        self.name, self.pool_rows, self.R, self.log, self.flips = name, slices * rays, rays, log, flips
        self.cursor = self.parity = self.steps_done = 0

    def before_step(self):
        if self.cursor >= self.pool_rows - self.R:
            self.cursor = 0
            self.log.append("S" + self.name)
        return -(-(self.pool_rows - self.R - self.cursor) // self.R)

    def record(self, slot, par):
        self.log.append((self.name, slot, par))

    def advance(self, U=1):
        self.cursor += U * self.R
        self.steps_done += U
        if self.flips:
            self.parity ^= U & 1

    def state(self):
        return self.cursor, self.steps_done, self.parity


class Replayable:
    def __init__(self, body, log):
        self.body, self.log = body, log

    def replay(self):
        self.log.append(("replay", self.body))


def make(sg, specs, warmup, unroll, layout="single"):
    """the real driver over fake branches ``specs`` = [(name, slices, rays)], its three device touch points recording"""
    log = []

    class Recording(sg.StepGraphs):
        def capture(self, fn, pool=None):
            start = len(log)
            fn()
            body = log[start:]
            del log[start:]
            return Replayable(body, log)

        @contextlib.contextmanager
        def fork(self):
            log.append("fork")
            yield
            log.append("back")

        def join(self):
            log.append("join")
    branches = [FakeBranch(name, slices, rays, log, flips=k == 0) for k, (name, slices, rays) in enumerate(specs)]
    return Recording(branches, warmup, unroll, layout=layout), branches, log


def bodies(entries, name):
    return [e for e in entries if isinstance(e, tuple) and e[0] == name]


def tokens(log, drv):
    """the log as the notation above; every graph body is checked on the way: U steps of every branch, the main branch's with
    history slots 0 .. U - 2, None and alternating parity"""
    out, main, k = [], drv.main.name, 0
    while k < len(log):
        e = log[k]
        k += 1
        if isinstance(e, str):
            if e.startswith("S"):
                out.append(e if drv.side is not None else "S")
        elif e[0] == "replay":
            mine = bodies(e[1], main)
            U, p = len(mine), mine[0][2]
            assert mine == [(main, i if i < U - 1 else None, p ^ (i & 1)) for i in range(U)]
            assert drv.side is None or len(bodies(e[1], drv.side.name)) == U
            out.append("g1@%d" % p if U == 1 else "%d@%d" % (U, p))
        elif e[0] == main:
            assert e[1] is None                    # an eager step writes no history slot
            out.append("e")
    return " ".join(out)


def run_calls(drv, log, calls, **kw):
    parts = []
    for n in calls:
        del log[:]
        drv.run(n, **kw)
        parts.append(tokens(log, drv))
    return " | ".join(parts)


ONE = "e e g1@0 | 6@1 2@1 g1@1 S 6@0 4@0 g1@0 | g1@1 | S 6@0 6@0 | S 6@0 6@0 S 6@0 6@0 S 6@0 6@0 S 2@0 g1@0"
TWO = "e e e 2@1 g1@1 Sb 4@0 So 2@0 Sb 6@0 Sb 2@0 So 4@0 Sb 6@0 So Sb 6@0 Sb g1@0"


def test_one_category_branch_sends_what_the_trainers_own_loop_sent(sg):
    """13 slices per epoch, unroll 6, two eager steps: the case of tests/test_trainer_gpu.py's multi-step test"""
    drv, (o,), log = make(sg, [("o", 13, 96)], warmup=2, unroll=6)
    assert run_calls(drv, log, (3, 20, 1, 12, 39)) == ONE
    assert o.state() == (3 * 96, 75, 1)
    single, (s,), _ = make(sg, [("o", 13, 96)], warmup=2, unroll=6)
    for _ in range(75):
        single.step()
    assert s.state() == o.state()


@pytest.mark.parametrize("unroll,want", [(None, TWO), (5, TWO.replace("6@0", "4@0 2@0"))])
def test_two_branches_stop_at_the_epoch_ends_of_both(sg, unroll, want):
    """category 11 slices, background 7, three eager iterations, groups of up to 8 (the category trainer allows 16): the case of
    tests/test_bg_fused_gpu.py's whole-iteration test; an odd ``unroll`` gives even groups"""
    drv, (o, b), log = make(sg, [("o", 11, 256), ("b", 7, 300)], warmup=3, unroll=16, layout="free")
    assert run_calls(drv, log, (37,), unroll=8 if unroll is None else unroll) == want
    assert o.state() == (7 * 256, 37, 1) and b.state() == (1 * 300, 37, 0)
    single, (so, sb), _ = make(sg, [("o", 11, 256), ("b", 7, 300)], warmup=3, unroll=16, layout="free")
    for _ in range(37):
        single.step()
    assert so.state() == o.state() and sb.state() == b.state()


def test_short_pools_send_small_groups_from_both_parities(sg):
    """category 7 slices, background 6, groups of up to 4: the case of tests/test_bg_fused_gpu.py's layout test"""
    drv, (o, b), log = make(sg, [("o", 7, 64), ("b", 6, 40)], warmup=3, unroll=16, layout="iter")
    assert run_calls(drv, log, (17,), unroll=4) == "e e e 2@1 Sb g1@1 So 4@0 Sb 2@0 So 2@0 g1@0 Sb 2@1"
    assert o.state() == (5 * 64, 17, 1) and b.state() == (2 * 40, 17, 0)


def test_what_a_group_of_four_records_in_each_layout(sg):
    o4 = [("o", 0, 0), ("o", 1, 1), ("o", 2, 0), ("o", None, 1)]
    b4 = [("b",) + s[1:] for s in o4]
    want = {"free": ["fork"] + b4 + ["back"] + o4 + ["join"],
            "iter": sum((["fork", b, "back", o, "join"] for o, b in zip(o4, b4)), []),
            "single": sum(([b, o] for o, b in zip(o4, b4)), [])}
    for layout, seq in want.items():
        drv, _, log = make(sg, [("o", 11, 256), ("b", 7, 300)], warmup=3, unroll=16, layout=layout)
        drv.record(0, 4)
        assert log == seq, layout
        assert (log.count("fork"), log.count("join")) == {"free": (1, 1), "iter": (4, 4), "single": (0, 0)}[layout]
    drv, _, log = make(sg, [("o", 11, 256)], warmup=2, unroll=16)          # one branch: its four bodies, from parity 1
    drv.record(1, 4)
    assert log == [("o", s, 1 ^ p) for _, s, p in o4]


def test_prepare_captures_every_graph_and_runs_none(sg):
    drv, _, log = make(sg, [("o", 13, 96)], warmup=2, unroll=6)
    drv.run(1)
    drv.prepare(6)
    assert drv.graphs == {}                                    # warm-up is not over
    drv.run(1)
    del log[:]
    drv.prepare(6)
    assert set(drv.graphs) == {0, 1, (0, 6), (0, 4), (0, 2), (1, 6), (1, 4), (1, 2)} and log == []
    assert [s[1:] for s in drv.graphs[(1, 4)].body] == [(0, 1), (1, 0), (2, 1), (None, 0)]
    drv.prepare(6, graph=False)
    none, _, _ = make(sg, [("o", 13, 96)], warmup=0, unroll=6)
    none.groups = False                                        # (around a gradient all-reduce)
    none.prepare(6)
    assert none.graphs == {}


def test_without_graphs_every_step_is_eager(sg):
    for specs, warmup in (([("o", 13, 96)], 2), ([("o", 11, 256), ("b", 7, 300)], 3)):
        drv, branches, log = make(sg, specs, warmup=warmup, unroll=6)
        drv.run(30, graph=False)
        drv.step(graph=False)
        assert drv.graphs == {} and not [e for e in log if e[0] == "replay"]
        assert all(len(bodies(log, b.name)) == 31 and b.steps_done == 31 for b in branches)


def test_a_single_step_hook_replaces_record_and_capture(sg):
    """the category trainer's two graphs around a gradient all-reduce: single steps through the hook, no groups"""
    drv, (o,), log = make(sg, [("o", 13, 96)], warmup=2, unroll=6)
    drv.groups, drv.single = False, lambda graph: log.append(("hook", graph))
    drv.run(5)
    drv.step()
    assert log == [("hook", False)] * 2 + [("hook", True)] * 4 and drv.graphs == {} and o.state() == (6 * 96, 6, 0)


def test_planner_alone(sg):
    gs = sg.group_sizes
    for left in range(2, 33):                      # what goes out in front of an epoch end `left` steps away
        assert left - sg.plan_group(32, left, 32, True) in (0, 1)
    for n in range(0, 24):
        for left in range(0, 24):
            for unroll in range(1, 20):
                U = sg.plan_group(n, left, unroll, True)
                assert U % 2 == 0 and U <= unroll and U <= n and U <= left and (U == 0 or U in gs(unroll))
                assert U + 2 > min(n, left, unroll)            # ... and the largest such
                assert sg.plan_group(n, left, unroll, False) == 0
