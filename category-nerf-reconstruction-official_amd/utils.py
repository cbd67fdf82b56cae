"""Ensemble glue with the reference's signature (src/utils.py:24-28).

``update_vmap(models, optimiser)`` stacks the per-class modules' parameters into ``(C, ...)`` leaves,
registers them as a new param group, and returns ``(fmodel, params, buffers)`` such that
``functorch.vmap(fmodel)(params, buffers, *stacked_inputs)`` -- the exact call at train.py:154-155 --
lands in the class-batched HIP kernels through the Functions' ``vmap`` rules (ops.py).
"""
import torch
from torch.func import functional_call, stack_module_state


def combine_state_for_ensemble(models):
    """(fmodel, params, buffers) like functorch's helper: params/buffers are tuples of stacked
    tensors in ``named_parameters()`` / ``named_buffers()`` order."""
    params, buffers = stack_module_state(models)
    pnames, bnames = list(params.keys()), list(buffers.keys())
    base = models[0]

    def fmodel(p, b, *args, **kwargs):
        state = {n: t for n, t in zip(pnames, p)}
        state.update({n: t for n, t in zip(bnames, b)})
        return functional_call(base, state, args, kwargs)

    return fmodel, tuple(params[n] for n in pnames), tuple(buffers[n] for n in bnames)


def update_vmap(models, optimiser):
    fmodel, params, buffers = combine_state_for_ensemble(models)
    [p.requires_grad_() for p in params]
    optimiser.add_param_group({"params": params})
    return (fmodel, params, buffers)


# ---- sim3 <-> 8-vector [scale, qw, qx, qy, qz, tx, ty, tz] ------------------------------------------------------------
# The form the reference keeps per object in ``sceneCategory.object_tensor_dict`` and writes into checkpoints
# (src/utils.py:367-447 get_tensor_from_transform_sim3 / get_transform_from_tensor_sim3; consumers read element 0 as the
# scale and elements 1: as quaternion + translation, train.py:231-234, src/scene_cateogries.py:378-379).
def get_tensor_from_transform_sim3(RT):
    """(4,4) sim3 (numpy or tensor) -> float32 tensor (8,).  scale = det(R s)^(1/3); the quaternion comes from scipy's
    Rotation (w first), the same third-party routine the reference calls, so the numbers are identical."""
    import numpy as np
    from scipy.spatial.transform import Rotation
    M = np.array(RT.detach().cpu().numpy() if torch.is_tensor(RT) else RT, dtype=np.float64)
    scale = np.linalg.det(M[:3, :3]) ** (1.0 / 3.0)
    scale32 = torch.tensor([scale], dtype=torch.float32)
    Rm = M[:3, :3] / scale32.numpy()                      # the reference divides by the float32 scale tensor
    x, y, z, w = Rotation.from_matrix(Rm).as_quat()
    vec = np.concatenate([[w, x, y, z], M[:3, 3]])
    return torch.cat([scale32, torch.from_numpy(vec).float()], 0)


def get_transform_from_tensor_sim3(vec):
    """(8,) or (n,8) [scale, qw, qx, qy, qz, t] -> (4,4) / (n,4,4) sim3 matrices (differentiable torch ops)."""
    single = vec.dim() == 1
    v = vec[None] if single else vec
    s, q, t = v[:, 0], v[:, 1:5], v[:, 5:8]
    qr, qi, qj, qk = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    R = torch.stack([1 - two_s * (qj * qj + qk * qk), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                     two_s * (qi * qj + qk * qr), 1 - two_s * (qi * qi + qk * qk), two_s * (qj * qk - qi * qr),
                     two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi * qi + qj * qj)],
                    -1).view(-1, 3, 3)
    T = torch.eye(4, device=v.device, dtype=v.dtype).repeat(v.shape[0], 1, 1)
    T[:, :3, :3] = R * s[:, None, None]
    T[:, :3, 3] = t
    return T[0] if single else T


def quad2rotation(quad):
    """(n,4) quaternions [r, i, j, k] (need not be unit) -> (n,3,3) rotations (src/utils.py:468-491)"""
    qr, qi, qj, qk = quad.unbind(-1)
    two_s = 2.0 / (quad * quad).sum(-1)
    return torch.stack([1 - two_s * (qj ** 2 + qk ** 2), two_s * (qi * qj - qk * qr), two_s * (qi * qk + qj * qr),
                        two_s * (qi * qj + qk * qr), 1 - two_s * (qi ** 2 + qk ** 2), two_s * (qj * qk - qi * qr),
                        two_s * (qi * qk - qj * qr), two_s * (qj * qk + qi * qr), 1 - two_s * (qi ** 2 + qj ** 2)],
                       -1).view(-1, 3, 3)


def get_transform_from_tensor(inputs):
    """(7,) or (n,7) [qr, qi, qj, qk, tx, ty, tz] -> (4,4) / (n,4,4) rigid transforms (src/utils.py:411-430; train.py:232 calls
    it on object_tensor_dict[obj][1:])."""
    single = inputs.dim() == 1
    v = inputs[None] if single else inputs
    RT = torch.eye(4, device=v.device, dtype=v.dtype).repeat(v.shape[0], 1, 1)
    RT[:, :3, :3] = quad2rotation(v[:, :4])
    RT[:, :3, 3] = v[:, 4:7]
    return RT[0] if single else RT


# ---- dataset helpers (src/utils.py:16-22, :30-51, :69-78, :322-327) ---------------------------------------------------
class BoundingBox():
    """An oriented 3-D box as the registration result stores it (bbox3D of inst_dict.pkl): extent, R, center, points3d (8,3)."""

    def __init__(self):
        super(BoundingBox, self).__init__()
        self.extent = None
        self.R = None
        self.center = None
        self.points3d = None


def enlarge_bbox(bbox, scale, w, h):
    """[min_x, min_y, max_x, max_y] grown by int(0.5 * scale * size) per side, clipped to [0, w-1] x [0, h-1]; None when either
    margin is 0.  Arithmetic is whatever the inputs carry: torch tensors (Replica) give float32 margins, ints give double."""
    assert scale >= 0
    import numpy as np
    min_x, min_y, max_x, max_y = bbox
    margin_x = int(0.5 * scale * (max_x - min_x))
    margin_y = int(0.5 * scale * (max_y - min_y))
    if margin_x == 0 or margin_y == 0:
        return None
    min_x, max_x = np.clip(min_x - margin_x, 0, w - 1), np.clip(max_x + margin_x, 0, w - 1)
    min_y, max_y = np.clip(min_y - margin_y, 0, h - 1), np.clip(max_y + margin_y, 0, h - 1)
    return [int(min_x), int(min_y), int(max_x), int(max_y)]


def get_bbox2d_batch(img):
    """(b, h, w) masks -> (rmins, rmaxs, cmins, cmaxs) int64: first row with a set pixel, one past the last, the same for
    columns (0 and h / w for an empty mask, as torch.argmax gives)."""
    b, h, w = img.shape[:3]
    rows, cols = torch.any(img, axis=2).float(), torch.any(img, axis=1).float()
    rmins = torch.argmax(rows, dim=1)
    rmaxs = h - torch.argmax(rows.flip(dims=[1]), dim=1)
    cmins = torch.argmax(cols, dim=1)
    cmaxs = w - torch.argmax(cols.flip(dims=[1]), dim=1)
    return rmins, rmaxs, cmins, cmaxs


def load_matrix_from_txt(path, shape=(4, 4)):
    """whitespace-separated floats of a text file -> float64 array of `shape`"""
    import numpy as np
    with open(path) as f:
        values = [float(v) for v in f.read().split()]
    return np.array(values).reshape(shape)
