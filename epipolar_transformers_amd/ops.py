"""Torch-facing wrappers of the C ABI (torch is plumbing: device memory, the
current HIP stream and autograd bookkeeping; all arithmetic of the path is in
the HIP library).  Feature tensors are logical NCHW like the reference's; their
memory is NHWC (torch.channels_last), converted once with our own kernel when a
caller hands NCHW-contiguous memory."""
from __future__ import annotations

import ctypes
import threading
import weakref
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import EtLayerDesc


@dataclass
class LayerSpec:
    """The static part of an EtLayerDesc + the three small constant arrays the
    reference builds in Epipolar.__init__ (epipolar.py:22-54)."""

    H: int
    W: int
    K: int
    downsample: float = 4.0
    image_resize: float = 1.0
    predict_resize: float = 1.0
    correct_normalize: bool = True
    align_corners: bool = False
    softmax_scale: float = 0.125
    softmax_enabled: bool = True
    eps: float = 0.001
    src_grad_mask: int = 3
    variant: int = 0

    def __post_init__(self):
        ds = self.downsample
        # pix2coord (multiview.py:154-157) * resize factors, same float32 op order as epipolar.py:35-38
        y = torch.arange(0, self.H, dtype=torch.float)
        x = torch.arange(0, self.W, dtype=torch.float)
        y = (y * ds + ds / 2.0 - 0.5) * self.image_resize * self.predict_resize
        x = (x * ds + ds / 2.0 - 0.5) * self.image_resize * self.predict_resize
        self.xs, self.ys = x.contiguous(), y.contiguous()
        # torch.range(0, 1, 1/(K-1)) (epipolar.py:54): start + i*step in double, rounded to float32
        step = 1.0 / (self.K - 1)
        self.steps = torch.from_numpy((np.arange(self.K, dtype=np.float64) * step).astype(np.float32))
        self._dev = {}

    def constants(self, device):
        """xs, ys, steps resident on `device` (uploaded once per device)."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(device) for t in (self.xs, self.ys, self.steps))
        return self._dev[key]

    def desc(self, N: int, C: int) -> EtLayerDesc:
        return EtLayerDesc(
            N=N, C=C, H=self.H, W=self.W, K=self.K,
            xmin=float(self.xs[0]), ymin=float(self.ys[0]), xmax=float(self.xs[-1]), ymax=float(self.ys[-1]),
            eps=self.eps, downsample=float(self.downsample), image_resize=float(self.image_resize),
            predict_resize=float(self.predict_resize), correct_normalize=int(self.correct_normalize),
            align_corners=int(self.align_corners), softmax_scale=float(self.softmax_scale),
            softmax_enabled=int(self.softmax_enabled), src_grad_mask=int(self.src_grad_mask),
            # (ET_VARIANT_BWD_DETERMINISTIC is read HERE, by backward_nhwc's choice of form; the kernels never see it, so the
            #  forward of a deterministic layer is the default forward)
            variant=int(self.variant) & ~_lib.ET_VARIANT_BWD_DETERMINISTIC)


def _require_gpu(t: torch.Tensor, name: str, dtype=torch.float32):
    if not t.is_cuda:
        raise _lib.EpipolarAmdError(
            "%s is on %s: the epipolar hot path runs on the GPU only (no CPU fallback)" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, str(dtype).replace("torch.", ""), t.dtype))


# The argument checks of every wrapper: the library takes raw addresses, so whatever it is to read or write is checked HERE for
# device, dtype, shape and contiguity (EpipolarAmdError off the GPU, TypeError for the dtype, ValueError for the rest), with
# raised errors -- `python -O` must not remove them.  `msg`: the ValueError's text where a wrapper has words of its own.
def _require_f32(t: torch.Tensor, name: str, device, shape=None, msg: str = None):
    """`t`: a contiguous float32 tensor on `device` (a GPU) -- of `shape` where one is given; (..., 256) fixes the last
    dimension only."""
    _require_gpu(t, name)
    ok = t.device == device and t.is_contiguous()
    if ok and shape is not None:
        ok = tuple(t.shape[-1:]) == tuple(shape[1:]) if shape[0] is Ellipsis else tuple(t.shape) == tuple(shape)
    if not ok:
        raise ValueError(msg or "%s must be a contiguous float32 tensor%s on %s, got %s on %s" % (
            name, "" if shape is None else " of shape %s" % (tuple(shape),), device, tuple(t.shape), t.device))


def _require_vector(t: torch.Tensor, name: str, n: int, device):
    """`t`: `n` contiguous float32 values on `device` (a per-channel vector, whatever its number of dimensions)."""
    _require_gpu(t, name)
    if t.numel() != n or not t.is_contiguous() or t.device != device:
        raise ValueError("%s must be a contiguous float32 vector of %d values on %s" % (name, n, device))


def _require_bytes(t: torch.Tensor, name: str, nbytes: int, device, msg: str = None):
    """`t`: a contiguous uint8 buffer of at least `nbytes` bytes on `device` (a workspace, a packed weight)."""
    _require_gpu(t, name, torch.uint8)
    if t.numel() < nbytes or not t.is_contiguous() or t.device != device:
        raise ValueError(msg or "%s must be a contiguous uint8 tensor of at least %d bytes on %s" % (name, nbytes, device))


def _require_cam(cam: torch.Tensor, n: int, device):
    _require_f32(cam, "cam", device, (n, _lib.ET_CAM_STRIDE), "cam must be a contiguous (N,%d) tensor" % _lib.ET_CAM_STRIDE)


def _stream(t: torch.Tensor):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _call(name: str, on, *args):
    """Call the library's export `name` with the device of `on` (a tensor or a device) current, and raise its error under that
    name.  `on` None: the caller holds the device guard itself (it has more to do under it)."""
    if on is None:
        return _lib.check(getattr(_lib.load(), name)(*args), name)
    with torch.cuda.device(on.device if isinstance(on, torch.Tensor) else on):
        _lib.check(getattr(_lib.load(), name)(*args), name)


POISON_OUTPUTS = False      # tests set this: every output buffer starts as NaN, so that a kernel that leaves part of its
                            # output unwritten cannot hide behind the (correct) values a recycled allocation still holds


def _empty(shape, like=None, device=None, dtype=torch.float32):
    if like is not None:
        shape, device, dtype = like.shape, like.device, like.dtype
    t = torch.empty(tuple(shape), dtype=dtype, device=device)
    if POISON_OUTPUTS and t.is_floating_point():
        t.fill_(float("nan"))
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def to_nhwc(x: torch.Tensor) -> torch.Tensor:
    """Logical (N,C,H,W) -> contiguous (N,H,W,C) memory.  Zero-copy when x is
    already channels_last; otherwise one pass of et_nchw_to_nhwc."""
    _require_gpu(x, "feature map")
    n, c, h, w = x.shape
    perm = x.permute(0, 2, 3, 1)
    if perm.is_contiguous():
        return perm
    src = x.contiguous()
    dst = _empty((n, h, w, c), device=x.device, dtype=x.dtype)
    _call("et_nchw_to_nhwc", x, n, c, h, w, _ptr(src), _ptr(dst), _stream(x))
    return dst


def to_nchw_contiguous(x_nhwc: torch.Tensor) -> torch.Tensor:
    """(N,H,W,C) memory -> NCHW-contiguous tensor via et_nhwc_to_nchw."""
    _require_gpu(x_nhwc, "feature map")
    n, h, w, c = x_nhwc.shape
    dst = _empty((n, c, h, w), device=x_nhwc.device, dtype=x_nhwc.dtype)
    _call("et_nhwc_to_nchw", x_nhwc, n, c, h, w, _ptr(x_nhwc.contiguous()), _ptr(dst), _stream(x_nhwc))
    return dst


def sample_locs(spec: LayerSpec, cam: torch.Tensor) -> torch.Tensor:
    """grid2sample_locs (epipolar.py:323-418): (K,N,H,W,2)."""
    _require_cam(cam, cam.shape[0], cam.device)
    n = cam.shape[0]
    xs, ys, steps = spec.constants(cam.device)
    out = _empty((spec.K, n, spec.H, spec.W, 2), device=cam.device)
    d = spec.desc(n, 4)
    _call("et_sample_locs", cam, ctypes.byref(d), _ptr(xs), _ptr(ys), _ptr(steps), _ptr(cam), _ptr(out), _stream(cam))
    return out


def _general_flags(pooling=False, prior_mul=False, cosine=False, attention_max=False, sim_prior=False) -> int:
    return ((_lib.ET_GENERAL_POOLING if pooling else 0) | (_lib.ET_GENERAL_PRIOR_MUL if prior_mul else 0) |
            (_lib.ET_GENERAL_COSINE if cosine else 0) | (_lib.ET_GENERAL_ATTENTION_MAX if attention_max else 0) |
            (_lib.ET_GENERAL_SIM_PRIOR if sim_prior else 0))


def _require_general(spec: LayerSpec, q, map_sim, map_val, cam, prior, pooling):
    """The arguments forward_general_nhwc and backward_general_nhwc share.  Returns (n, h, w, cs, cv, K')."""
    for t, nm in ((q, "q"), (map_sim, "map_sim"), (map_val, "map_val")):
        _require_f32(t, nm, q.device, msg="q / map_sim / map_val must be contiguous (N,H,W,C) tensors")
    n, h, w, cs = q.shape
    if (h, w) != (spec.H, spec.W) or map_sim.shape != q.shape or map_val.dim() != 4 or map_val.shape[:3] != q.shape[:3]:
        raise ValueError("maps %s / %s / %s do not match the layer's %dx%d" %
                         (tuple(q.shape), tuple(map_sim.shape), tuple(map_val.shape), spec.H, spec.W))
    _require_cam(cam, n, q.device)
    ks = spec.K // 2 if pooling else spec.K
    if prior is not None:
        _require_f32(prior, "prior", q.device, (n, ks, h, w),
                     "prior must be (N,K',H,W) = %s, got %s" % ((n, ks, h, w), tuple(prior.shape)))
    return n, h, w, cs, map_val.shape[-1], ks


def forward_general_nhwc(spec: LayerSpec, q: torch.Tensor, map_sim: torch.Tensor, map_val: torch.Tensor, cam: torch.Tensor,
                         prior: torch.Tensor = None, pooling=False, prior_mul=False, cosine=False, attention_max=False,
                         want_attn=True, want_corr=True, sim_prior=False):
    """The operator's parameterised / pooled / prior branches as ONE kernel (et_epipolar_forward_general; forward only).
    q, map_sim: (N,H,W,Cs); map_val: (N,H,W,Cv), channels last, contiguous; prior: (N,K',H,W) or None, K' = K/2 with
    `pooling` (epipolar.py:200-202), else K.  Returns out (N,H,W,Cv), attn (N,K',H,W)|None, corr_pos (N,H,W,2)|None."""
    n, h, w, cs, cv, ks = _require_general(spec, q, map_sim, map_val, cam, prior, pooling)
    xs, ys, steps = spec.constants(q.device)
    out = _empty((n, h, w, cv), device=q.device)
    attn = _empty((n, ks, h, w), device=q.device) if want_attn else None
    corr = _empty((n, h, w, 2), device=q.device) if want_corr else None
    flags = _general_flags(pooling, prior_mul, cosine, attention_max, sim_prior)
    d = spec.desc(n, 4)
    _call("et_epipolar_forward_general", q, ctypes.byref(d), _ptr(xs), _ptr(ys), _ptr(steps), _ptr(cam), _ptr(q), _ptr(map_sim),
          _ptr(map_val), _ptr(prior), cs, cv, flags, _ptr(out), _ptr(attn), _ptr(corr), _stream(q))
    return out, attn, corr


def _require_grad_attn(grad_attn, shape, device):
    """`grad_attn`: None, or d loss / d attn -- float32 of the attention's shape on `device`; returned contiguous."""
    if grad_attn is None:
        return None
    _require_gpu(grad_attn, "grad_attn")
    if tuple(grad_attn.shape) != tuple(shape) or grad_attn.device != device:
        raise ValueError("grad_attn must be a float32 %s tensor on %s, got %s on %s" %
                         (tuple(shape), device, tuple(grad_attn.shape), grad_attn.device))
    return grad_attn.contiguous()


def backward_general_nhwc(spec: LayerSpec, q, map_sim, map_val, cam, grad_out, pooling=False, need_sim=True, need_val=True,
                          prior=None, prior_mul=False, cosine=False, attention_max=False, sim_prior=False, need_prior=False,
                          grad_attn=None):
    """Backward of forward_general_nhwc, every branch: returns (grad_q, grad_map_sim | None, grad_map_val | None,
    grad_prior | None), NHWC maps, grad_prior (N,K',H,W).  The map gradients are accumulated with float atomics
    (reproducible to rounding only).  `grad_attn`: d loss / d attn (N,K',H,W) or None -- the gradient through the returned
    attention (et_epipolar_backward_general_ga)."""
    n, h, w, cs, cv, ks = _require_general(spec, q, map_sim, map_val, cam, prior, pooling)
    _require_f32(grad_out, "grad_out", q.device, (n, h, w, cv), "grad_out must be a contiguous (N,H,W,Cv) tensor")
    grad_attn = _require_grad_attn(grad_attn, (n, ks, h, w), q.device)
    xs, ys, steps = spec.constants(q.device)
    gq = _empty(None, like=q)
    gsim = torch.zeros_like(map_sim) if need_sim else None
    gval = torch.zeros_like(map_val) if need_val else None
    gprior = _empty(None, like=prior) if (need_prior and prior is not None) else None
    d = spec.desc(n, 4)
    flags = _general_flags(pooling, prior_mul, cosine, attention_max, sim_prior)
    _call("et_epipolar_backward_general_ga", q, ctypes.byref(d), _ptr(xs), _ptr(ys), _ptr(steps), _ptr(cam), _ptr(q), _ptr(map_sim),
          _ptr(map_val), _ptr(prior), _ptr(grad_out), _ptr(grad_attn), cs, cv, flags, _ptr(gq), _ptr(gsim), _ptr(gval), _ptr(gprior),
          _stream(q))
    return gq, gsim, gval, gprior


class GeneralAttend(torch.autograd.Function):
    """The operator's non-headline branches with autograd (every one since ABI 12): logical NCHW in and out, `prior` the
    (N,K',H,W) stack of the pairs' prior tables or None; `corr_pos` without gradient, `attn` too unless `attn_grad` (as
    EpipolarAttend).  `mode`: dict(pooling, prior_mul, cosine, attention_max, sim_prior) of bools."""

    @staticmethod
    def forward(ctx, q, map_sim, map_val, cam, spec: LayerSpec, pooling, prior=None, mode=None, attn_grad: bool = False):
        mode = dict(mode or {}, pooling=bool(pooling))
        qn, m1, m2 = to_nhwc(q), to_nhwc(map_sim), to_nhwc(map_val)
        pr = None if prior is None else prior.contiguous()
        out, attn, corr = forward_general_nhwc(spec, qn, m1, m2, cam, prior=pr, **mode)
        ctx.spec, ctx.mode, ctx.has_prior = spec, mode, pr is not None
        ctx.save_for_backward(*((qn, m1, m2, cam) + ((pr,) if pr is not None else ())))
        _mark_attention(ctx, attn, corr, attn_grad)
        return out.permute(0, 3, 1, 2), attn, corr

    @staticmethod
    def backward(ctx, grad_out, grad_attn, _gc):
        qn, m1, m2, cam = ctx.saved_tensors[:4]
        if grad_out is None:                # (attn_grad: a loss on the attention alone)
            grad_out = torch.zeros_like(m2).permute(0, 3, 1, 2)
        pr = ctx.saved_tensors[4] if ctx.has_prior else None
        if (ctx.spec.variant & _lib.ET_VARIANT_BWD_DETERMINISTIC) and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            raise RuntimeError("EPIPOLAR_AMD.DETERMINISTIC: the option branches (theta / phi / g, POOLING, PRIOR, cosine, ATTENTION max, "
                               "supplied depth) accumulate the gradient of a sampled map with float atomics "
                               "(et_epipolar_backward_general), which is not bit-reproducible; only the headline mode has a "
                               "deterministic backward")
        gq, gs, gv, gp = backward_general_nhwc(ctx.spec, qn, m1, m2, cam, to_nhwc(grad_out), need_sim=ctx.needs_input_grad[1],
                                               need_val=ctx.needs_input_grad[2], prior=pr,
                                               need_prior=ctx.has_prior and ctx.needs_input_grad[6],
                                               grad_attn=grad_attn if ctx.attn_grad else None,
                                               **ctx.mode)
        nchw = lambda t: None if t is None else t.permute(0, 3, 1, 2)
        return nchw(gq) if ctx.needs_input_grad[0] else None, nchw(gs), nchw(gv), None, None, None, gp, None, None


def _mark_attention(ctx, attn, corr, attn_grad: bool):
    """Which of the two side outputs of the attend functions carry gradient.  Default: neither.  `attn_grad`: the attention does
    (the reference's `depth` is an ordinary autograd tensor, epipolar.py:245, 263) -- and gradients are no longer materialised,
    so that an attention nobody differentiated arrives in backward as None (today's path, no zero tensor) and a loss on the
    attention alone hands a None grad_out (replaced by zeros there)."""
    ctx.attn_grad = bool(attn_grad)         # (backward reads grad_attn only then: a non-differentiable output's is zeros or None)
    if attn_grad:
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(corr)
    else:
        ctx.mark_non_differentiable(attn, corr)


_TILE_BITS = (_lib.ET_VARIANT_TILE_SPLIT | _lib.ET_VARIANT_TILE_CLASSIC |
              _lib.ET_VARIANT_WS_SETPRIO | _lib.ET_VARIANT_TILE_EXACT | _lib.ET_VARIANT_WS_BAND | _lib.ET_VARIANT_BWD_SPLIT_IN_PLACE)   # bits that tune the tile path instead of leaving it


def _require_pair(spec: LayerSpec, ref, src, cam, c: int = None, ref_index=None, src_index=None):
    """feat_ref / feat_src / cam of the headline entry points: contiguous (N,H,W,C) maps of the layer's size (with `c` channels,
    where the kernel is written for one width) and their (N,27) algebra, on one GPU.  With an index (the device copy
    _pair_indices returns) that operand is a POOL of any number of maps and N is the number of cameras.  Returns (n, h, w, c)."""
    for t, nm in ((ref, "feat_ref"), (src, "feat_src")):
        _require_f32(t, nm, ref.device, msg="feat_ref / feat_src must be contiguous (N,H,W,C) tensors")
    indexed = ref_index is not None or src_index is not None
    if ref.dim() != 4 or src.dim() != 4:
        raise ValueError("feat_ref / feat_src must be contiguous (N,H,W,C) tensors")
    n, (_, h, w, ch) = (cam.shape[0] if indexed else ref.shape[0]), ref.shape
    if ((h, w) != (spec.H, spec.W) or src.shape[1:] != ref.shape[1:] or (c is not None and ch != c) or
            (ref_index is None and ref.shape[0] != n) or (src_index is None and src.shape[0] != n)):
        raise ValueError("feature maps %s / %s do not match the layer's %dx%d%s%s" %
                         (tuple(ref.shape), tuple(src.shape), spec.H, spec.W, "" if c is None else " x %d" % c,
                          " (%d pairs; an operand without an index holds one map per pair)" % n if indexed else ""))
    _require_cam(cam, n, ref.device)
    return n, h, w, ch


# ---- pairs named by index into a stack of maps (ET_HAS_PAIR_INDEX) -----------------------------------------------------------
# The *_ix entry points read pair n's maps as feat_ref[ref_index[n]] / feat_src[src_index[n]] from two POOLS (they may be one
# tensor) instead of from private per-pair copies.  forward_nhwc / forward_fused_nhwc / backward_nhwc take the indices as CPU
# integer tensors or sequences: checked on the HOST (length N, integer dtype, range: ValueError), uploaded once and cached by
# value.  Where the indexed kernels do not apply (pair_index_applies), or the index is a CUDA tensor (its values are not on the
# host: checking them would synchronise), the same call gathers the pairs' maps with torch and runs the unindexed kernels.
PAIR_INDEX_FORMS = ("forward", "fused", "tile", "tile_det", "gather", "atomic", "pixel", "general")


def pair_index_applies(spec: LayerSpec, c: int, form: str) -> bool:
    """True when a call of `form` on `c` channels runs the indexed tile kernels; False = the gathered route (same results).
    `form`: "forward" (forward_nhwc), "fused" (forward_fused_nhwc), a backward form of backward_nhwc ("tile": indexed;
    "tile_det", "gather", "atomic": not), "pixel" (the per-pixel forward) or "general" (a mode of the general kernels).
    False for C != 256, a deterministic spec (ET_VARIANT_BWD_DETERMINISTIC), a variant bit that selects the per-pixel kernels,
    and any shape the tile path does not take."""
    if form not in PAIR_INDEX_FORMS:
        raise ValueError("unknown form %r (one of %s)" % (form, ", ".join(PAIR_INDEX_FORMS)))
    if c != 256 or form not in ("forward", "fused", "tile"):
        return False
    if spec.variant & _lib.ET_VARIANT_BWD_DETERMINISTIC:
        return False
    if form == "tile" and (spec.variant & _BWD_EXPLICIT):
        return False
    if form != "tile" and (spec.variant & ~_TILE_BITS) != 0:
        return False
    if form == "fused":
        return fused_layer_applies(spec, c)
    d = spec.desc(1, c)
    return int(_lib.load().et_epipolar_forward_workspace_bytes(ctypes.byref(d))) > 0


def check_pair_index(index, name: str, n: int, m: int) -> np.ndarray:
    """`index` (a CPU integer tensor or a sequence of ints) as a contiguous int32 array, after the checks the kernels rely on:
    one dimension of length `n`, an integer dtype, every value in [0, m).  Host work only; raises ValueError."""
    if torch.is_tensor(index):
        if index.is_cuda:
            raise ValueError("%s is a CUDA tensor: its values cannot be checked without a synchronisation" % name)
        if index.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError("%s must have an integer dtype, got %s" % (name, index.dtype))
        arr = index.detach().numpy()
    else:
        arr = np.asarray(index)
        if arr.size and arr.dtype.kind not in "iu":
            raise ValueError("%s must hold integers, got dtype %s" % (name, arr.dtype))
    if arr.ndim != 1 or arr.shape[0] != n:
        raise ValueError("%s must name one map per pair: length %d, got shape %s" % (name, n, tuple(arr.shape)))
    if n and (int(arr.min()) < 0 or int(arr.max()) >= m):
        raise ValueError("%s has values in [%d, %d]: outside the pool's %d maps" % (name, int(arr.min()), int(arr.max()), m))
    return np.ascontiguousarray(arr, dtype=np.int32)


class PairIndexCache:
    """Device copies of pair tables, keyed by VALUE (the bytes of the int32 array and the device) like camera.PairAlgebraCache:
    a model hands the same table every step, a recycled host address with other values must not hit."""

    def __init__(self, max_entries: int = 16):
        self.max_entries = max_entries
        self._store = {}
        self._lock = threading.Lock()

    def get(self, arr: np.ndarray, device) -> torch.Tensor:
        key = (arr.tobytes(), str(device))
        with self._lock:
            hit = self._store.get(key)
            if hit is None:
                hit = torch.from_numpy(arr.copy()).pin_memory().to(device, non_blocking=True)
                if len(self._store) >= self.max_entries:
                    self._store.pop(next(iter(self._store)))
                self._store[key] = hit
        return hit


_pair_index_cache = PairIndexCache()


def _is_device_index(index) -> bool:
    return torch.is_tensor(index) and index.is_cuda


def _as_torch_index(idx: torch.Tensor) -> torch.Tensor:
    """An index tensor index_select / index_add_ accept (int32 or int64; a caller's CUDA index may be narrower)."""
    return idx if idx.dtype in (torch.int32, torch.int64) else idx.long()


def device_pair_index(index, name: str, n: int, m: int, device) -> torch.Tensor:
    """The pair table on `device`: a CUDA tensor as it is (unchecked), anything else checked and uploaded through the cache."""
    if _is_device_index(index):
        return index
    return _pair_index_cache.get(check_pair_index(index, name, n, m), device)


def gather_pairs(pool: torch.Tensor, index, name: str = "index") -> torch.Tensor:
    """The gathered route: pool[index] along dimension 0 (`pool` as it is for a None index).  Differentiable torch op."""
    if index is None:
        return pool
    idx = device_pair_index(index, name, len(index), pool.shape[0], pool.device)
    return pool.index_select(0, _as_torch_index(idx))


def _pair_indices(spec: LayerSpec, ref, src, cam, ref_index, src_index, form: str):
    """What forward_nhwc / forward_fused_nhwc / backward_nhwc do with their index arguments, first of all: the host checks
    (ValueError, before anything touches the device), then the route.  Returns (ref, src, ref_index, src_index): the pools with
    the device copies of the indices (indexed kernels), or the gathered maps with (None, None)."""
    if ref_index is None and src_index is None:
        return ref, src, None, None
    n = cam.shape[0]
    for t, nm in ((ref, "feat_ref"), (src, "feat_src")):
        if not torch.is_tensor(t) or t.dim() != 4:
            raise ValueError("%s must be a contiguous (M,H,W,C) pool of maps" % nm)
    host = [None if idx is None or _is_device_index(idx) else check_pair_index(idx, nm, n, pool.shape[0])
            for idx, nm, pool in ((ref_index, "ref_index", ref), (src_index, "src_index", src))]
    _require_gpu(ref, "feat_ref")
    _require_gpu(src, "feat_src")
    dev = [idx if idx is None or _is_device_index(idx) else _pair_index_cache.get(h, ref.device)
           for idx, h in zip((ref_index, src_index), host)]
    if _is_device_index(ref_index) or _is_device_index(src_index) or not pair_index_applies(spec, ref.shape[-1], form):
        take = lambda pool, idx: pool if idx is None else pool.index_select(0, _as_torch_index(idx))
        return take(ref, dev[0]), take(src, dev[1]), None, None
    return ref, src, dev[0], dev[1]


def _ix_args(ref, src, ref_index, src_index):
    """The four trailing arguments of an *_ix entry point."""
    return _ptr(ref_index), _ptr(src_index), int(ref.shape[0]), int(src.shape[0])


def forward_nhwc(spec: LayerSpec, ref: torch.Tensor, src: torch.Tensor, cam: torch.Tensor,
                 want_attn=True, want_corr=True, res_bias=None, want_res_base=False, workspace=None,
                 ref_index=None, src_index=None):
    """ref/src: (N,H,W,C) contiguous.  Returns out (N,H,W,C), attn (N,K,H,W)|None, corr_pos (N,H,W,2)|None
    [, res_base (N,H,W,C) = ref + res_bias when want_res_base].  `workspace`: a caller-owned uint8 tensor for the
    tile path (see tile_workspace / tile_stats) instead of the cached per-(device, stream) one.
    `ref_index` / `src_index` (CPU integer tensors or sequences of N = cam.shape[0] values, each optional): ref / src are then
    POOLS (M,H,W,C) and pair n reads ref[ref_index[n]], src[src_index[n]] -- in place (et_epipolar_forward_tiled_ix) where
    pair_index_applies, from torch-gathered copies otherwise; the outputs stay per pair."""
    ref, src, ref_index, src_index = _pair_indices(spec, ref, src, cam, ref_index, src_index, "forward")
    n, h, w, c = _require_pair(spec, ref, src, cam, ref_index=ref_index, src_index=src_index)
    if res_bias is not None:
        if not want_res_base:
            raise ValueError("res_bias is added into res_base: it needs want_res_base")
        _require_vector(res_bias, "res_bias", c, ref.device)
    xs, ys, steps = spec.constants(ref.device)
    out = _empty((n, h, w, c), device=ref.device)
    attn = _empty((n, spec.K, h, w), device=ref.device) if want_attn else None
    corr = _empty((n, h, w, 2), device=ref.device) if want_corr else None
    base = _empty((n, h, w, c), device=ref.device) if want_res_base else None
    d = spec.desc(n, c)
    # variant 0 (the library default) takes the MFMA tile formulation wherever it applies (C == 256 head);
    # any explicit variant bit selects the per-pixel kernels
    ws_bytes = int(_lib.load().et_epipolar_forward_workspace_bytes(ctypes.byref(d))) if (d.variant & ~_TILE_BITS) == 0 else 0
    args = (ctypes.byref(d), _ptr(xs), _ptr(ys), _ptr(steps), _ptr(cam), _ptr(ref), _ptr(src), _ptr(out), _ptr(attn), _ptr(corr),
            _ptr(res_bias), _ptr(base))
    if ws_bytes > 0:
        ws = workspace if workspace is not None else _workspace(ref.device, ws_bytes, "fwd")
        _require_bytes(ws, "workspace", ws_bytes, ref.device,
                       "workspace of %d bytes on %s: need %d on %s" % (ws.numel(), ws.device, ws_bytes, ref.device))
        if ref_index is not None or src_index is not None:
            _call("et_epipolar_forward_tiled_ix", ref, *args, _ptr(ws), ctypes.c_size_t(ws_bytes), _stream(ref),
                  *_ix_args(ref, src, ref_index, src_index))
        else:
            _call("et_epipolar_forward_tiled", ref, *args, _ptr(ws), ctypes.c_size_t(ws_bytes), _stream(ref))
        if POISON_OUTPUTS:          # (test suite: surface a device-side fault at the call that caused it)
            check_tile_errors(workspace=ws)
    else:
        _call("et_epipolar_forward", ref, *args, _stream(ref))
    if want_res_base:
        return out, attn, corr, base
    return out, attn, corr


def fused_layer_applies(spec: LayerSpec, c: int, n: int = 1) -> bool:
    """True when et_epipolar_forward_fused covers this shape (the warp-specialised tile kernel: C == 256, maps up to
    96 x 96, K <= 64, soft-max on, no variant bit that leaves that kernel)."""
    allowed = _lib.ET_VARIANT_TILE_SPLIT | _lib.ET_VARIANT_WS_SETPRIO | _lib.ET_VARIANT_WS_BAND | _lib.ET_VARIANT_BWD_DETERMINISTIC
    if not (c == 256 and 2 <= spec.W <= 96 and spec.H <= 96 and spec.K <= 64 and spec.softmax_enabled and
            (spec.variant & ~allowed) == 0):
        return False
    d = spec.desc(n, c)
    return int(_lib.load().et_epipolar_forward_workspace_bytes(ctypes.byref(d))) > 0


def forward_fused_nhwc(spec: LayerSpec, ref: torch.Tensor, src: torch.Tensor, cam: torch.Tensor, packed: torch.Tensor,
                       bias: torch.Tensor, want_attn=True, want_corr=True, want_out=False, workspace=None,
                       ref_index=None, src_index=None):
    """The eval-mode layer as one data kernel (et_epipolar_forward_fused): returns x = ref + bias + out @ Wf^T (N,H,W,C),
    attn (N,K,H,W)|None, corr_pos (N,H,W,2)|None [, out when want_out].  `packed`: residual_gemm_pack(Wf).
    `ref_index` / `src_index`: as forward_nhwc's (et_epipolar_forward_fused_ix: the ref row of x through ref_index)."""
    ref, src, ref_index, src_index = _pair_indices(spec, ref, src, cam, ref_index, src_index, "fused")
    n, h, w, c = _require_pair(spec, ref, src, cam, c=256, ref_index=ref_index, src_index=src_index)
    lib = _lib.load()
    need = int(lib.et_residual_gemm_packed_bytes())
    _require_bytes(packed, "packed", need, ref.device, "packed holds %d bytes on %s: the kernel reads %d on %s (ops.residual_gemm_pack)" %
                   (packed.numel(), packed.device, need, ref.device))
    _require_vector(bias, "bias", c, ref.device)
    if workspace is not None:
        _require_bytes(workspace, "workspace", 0, ref.device, "workspace must be a uint8 tensor on %s" % (ref.device,))
    xs, ys, steps = spec.constants(ref.device)
    x = _empty((n, h, w, c), device=ref.device)
    # `out`: requested -> a fresh tensor; otherwise scratch for the rows of overflow tiles only (normally none is written),
    # one buffer per (device, stream) like the workspace: all use is stream-ordered
    out = _empty((n, h, w, c), device=ref.device) if want_out else _workspace(ref.device, x.numel() * 4, "fwd_out_scratch").view(torch.float32)[:x.numel()]
    attn = _empty((n, spec.K, h, w), device=ref.device) if want_attn else None
    corr = _empty((n, h, w, 2), device=ref.device) if want_corr else None
    d = spec.desc(n, c)
    ws_bytes = int(lib.et_epipolar_forward_workspace_bytes(ctypes.byref(d)))
    with torch.cuda.device(ref.device):             # (held here: the poll asks about the CURRENT device's stream)
        ws = workspace if workspace is not None else _workspace(ref.device, max(ws_bytes, 1), "fwd")
        indexed = ref_index is not None or src_index is not None
        _call("et_epipolar_forward_fused_ix" if indexed else "et_epipolar_forward_fused", None, ctypes.byref(d), _ptr(xs), _ptr(ys),
              _ptr(steps), _ptr(cam), _ptr(ref), _ptr(src), _ptr(packed), _ptr(bias), _ptr(x), _ptr(attn), _ptr(corr), _ptr(out),
              1 if want_out else 0, _ptr(ws), ctypes.c_size_t(ws.numel()), _stream(ref),
              *(_ix_args(ref, src, ref_index, src_index) if indexed else ()))
        if POISON_OUTPUTS:
            check_tile_errors(workspace=ws)
        else:
            _poll_tile_error(ws)
    return (x, attn, corr, out) if want_out else (x, attn, corr)


_workspaces = {}
_workspaces_lock = threading.Lock()


def _prune_dead_threads_locked():
    """Entries of host threads that no longer exist (nn.DataParallel starts new forward threads on every call): dropped, so
    the cache does not grow with the number of calls.  Caller holds _workspaces_lock."""
    alive = {t.ident for t in threading.enumerate()}
    for key in [k for k in _workspaces if k[4] not in alive]:
        del _workspaces[key]


def _workspace(device, nbytes: int, tag: str = "bwd") -> torch.Tensor:
    """Device scratch the library asks for (it allocates nothing itself): the pixel order / overflow list / tile
    statistics of the tile kernels (tag "fwd", 2.3 MB at Config 2) and the coefficient entries of the gather-form
    backward (tag "bwd", 3.8 GB at Config 2 -- sized for 288 GB of HBM).  One buffer per (device, stream, tag, host
    thread), grown on demand: all use is stream-ordered on the stream it is keyed by, and two host threads that launch
    on the SAME device and stream (nn.DataParallel replicas pinned to one GPU) get buffers of their own -- the cache is
    the package's only process-wide mutable state (guarded by a lock; entries of threads that have exited are dropped
    whenever a buffer is created), and no two callers ever write the same entry.  release_workspaces() drops them.

    What the kernels rely on (include/epipolar_amd.h; pinned by tests/test_gpu_workspace_contracts.py and
    tests/test_gpu_redzones.py): of the "fwd" buffer ONE word must not hold stale bits -- word 1 of its 64-word header, the
    sticky error word -- which is why a buffer is created zeroed and grows by swapping in a new zeroed tensor, never by
    clearing.  Header words 0 and 2..9 are cleared by every tile call before it uses them, everything behind the header is
    written before it is read, so the forward, the one-kernel layer and the tiled backward of any shape may follow each other
    on one buffer; the "bwd" / "zstats" / "zbwd" / "zwgrad" buffers may hold anything.  The base need not be 256-byte aligned
    (the library rounds it up and the sizes include the 256 bytes), and no kernel writes outside the bytes it was given."""
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(dev).cuda_stream, tag, threading.get_ident())
    with _workspaces_lock:
        buf = _workspaces.get(key)
        if buf is None or buf.numel() < nbytes:
            _prune_dead_threads_locked()
            # zero-initialised ONCE (include/epipolar_amd.h): the tile forward keeps a sticky error word in it
            _workspaces[key] = buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
    return buf


def _own_workspace(workspace, nbytes: int, device, tag: str):
    """The caller-owned workspace, checked -- or, when the caller gave none, the cached buffer of `tag`."""
    if workspace is None:
        return _workspace(device, nbytes, tag)
    _require_bytes(workspace, "workspace", nbytes, device)
    return workspace


# The 64-word int32 header at the 256-byte-aligned base of a tile workspace (include/epipolar_amd.h, csrc/et_tile_host.h), read
# HERE and nowhere else in the binding.  The words it uses:
_HEADER_WORDS = 64
_HEADER_DEFERRED = 0        # overflow / deferred count of the last tile call
_HEADER_ERROR = 1           # the sticky error word (et_epipolar_forward_workspace_error_offset: 4 bytes in, whatever the shape)
_HEADER_DIAGNOSTICS = 8     # words 0..7: what backward_deferred_tiles(header=True) returns


def _aligned_base(buf: torch.Tensor) -> int:
    return (-buf.data_ptr()) % 256                        # the library aligns the base up to 256 bytes


def _header(buf: torch.Tensor) -> torch.Tensor:
    """The header of the workspace `buf` as an int32 view (no copy, no synchronisation)."""
    base = _aligned_base(buf)
    return buf[base: base + 4 * _HEADER_WORDS].view(torch.int32)


def _read_tile_error(buf: torch.Tensor) -> int:
    return int(_header(buf)[_HEADER_ERROR].item())


_TILE_ERROR_TEXT = ("the tile kernels reported device-side error bits 0x%x (bit 1: a matrix wave of et_epipolar_forward_fused gave "
                    "up at the barrier in front of its third GEMM; bit 2: the deterministic tiled backward met a d(feat_src) "
                    "contribution beyond its fixed-point range -- the guard behind the quantum's bound, e.g. non-finite inputs -- and "
                    "did not add it; the results of that call are invalid)")


def _clear_tile_error(buf: torch.Tensor):
    _header(buf)[_HEADER_ERROR:_HEADER_ERROR + 1].zero_()


def check_tile_errors(spec: "LayerSpec" = None, n: int = None, c: int = 256, workspace: torch.Tensor = None, reset: bool = True):
    """Read the sticky error word the tile forward keeps in its workspace (the library never synchronises, so this is
    where a device-side fault surfaces: it synchronises).  Without arguments: every cached forward workspace; with
    `workspace`: that one (spec / n / c are accepted for compatibility; the word sits in the workspace header, at the same
    offset for every shape).  Raises EpipolarAmdError; with `reset` (default) the word is cleared once it has been
    reported, so that later calls are judged on their own.  Called after every tile forward when POISON_OUTPUTS is set
    (the test suite) and once per bench.py run; the product path (forward_fused_nhwc) polls the word without
    synchronising, see _poll_tile_error."""
    if workspace is not None:
        bufs = [workspace]
    else:
        with _workspaces_lock:      # (other threads may insert meanwhile: iterate over a snapshot)
            bufs = [buf for key, buf in list(_workspaces.items()) if key[3] == "fwd"]
    for buf in bufs:
        if buf is None or buf.numel() < 512:
            continue
        word = _read_tile_error(buf)
        if word:
            if reset:
                _clear_tile_error(buf)
            raise _lib.EpipolarAmdError(_TILE_ERROR_TEXT % word)


_TILE_ERROR_POLL_EVERY = 16


class _ErrorProbe:
    """Per-workspace state of the asynchronous poll: calls since the last probe, ONE pinned host word (allocated with the
    probe, not per poll) and the event behind the copy in flight (None: no copy pending)."""
    __slots__ = ("calls", "host", "event")

    def __init__(self):
        self.calls, self.host, self.event = 0, None, None


# The probe hangs on the workspace TENSOR itself (an attribute: a freed workspace takes its probe with it, and a new tensor that
# happens to get the same address starts from a clean state; a dictionary keyed by tensors would compare them element-wise).
_PROBE_ATTR = "_et_error_probe"


def _poll_tile_error(buf: torch.Tensor):
    """The product path's check of the sticky error word WITHOUT a host synchronisation: every 16th one-kernel forward on a
    workspace enqueues a 4-byte device-to-host copy of the word behind the kernel (pinned memory, non-blocking) and an
    event; a later call that finds the event complete reads the host copy and raises (and clears the word) if a wave
    of an EARLIER call gave up at its barrier.  A fault therefore surfaces at most ~32 calls late instead of never;
    check_tile_errors() is the immediate, synchronising form.
    Nothing happens while the stream is being captured into a graph: a copy or an event record would become part of the
    graph, and querying an event is not allowed during a global-mode capture (it invalidates the capture).  A replayed graph
    is therefore not polled -- call check_tile_errors() after a batch of replays."""
    if torch.cuda.is_current_stream_capturing():
        return
    st = getattr(buf, _PROBE_ATTR, None)
    if st is None:
        st = _ErrorProbe()
        setattr(buf, _PROBE_ATTR, st)
    if st.event is not None and st.event.query():
        word = int(st.host.item())
        st.event = None
        if word:
            _clear_tile_error(buf)
            raise _lib.EpipolarAmdError((_TILE_ERROR_TEXT % word) + " -- reported by the asynchronous poll: the faulty call is "
                                        "one of the last %d on this workspace" % (2 * _TILE_ERROR_POLL_EVERY))
    st.calls += 1
    if st.event is None and st.calls >= _TILE_ERROR_POLL_EVERY:
        st.calls = 0
        if st.host is None:
            st.host = torch.empty(1, dtype=torch.int32).pin_memory()
        st.host.copy_(_header(buf)[_HEADER_ERROR:_HEADER_ERROR + 1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(buf.device))
        st.event = ev


def release_workspaces():
    """Drop every cached scratch buffer (e.g. the 3.8 GB of the gather-form backward after a training phase)."""
    with _workspaces_lock:
        _workspaces.clear()
    _last_tile_backward_ws.clear()


def tile_workspace(spec: LayerSpec, n: int, c: int, device) -> torch.Tensor:
    """A caller-owned workspace for forward_nhwc(..., workspace=...) on the tile path (empty tensor if it does not
    apply to this shape)."""
    d = spec.desc(n, c)
    return torch.zeros(int(_lib.load().et_epipolar_forward_workspace_bytes(ctypes.byref(d))), dtype=torch.uint8,
                       device=device)


def tile_stats(spec: LayerSpec, n: int, c: int, workspace: torch.Tensor) -> torch.Tensor:
    """Per-tile statistics the tile forward leaves in its workspace: int32 (N * tiles_per_pair,),
    U | groups << 16 (size of the tile's source-row set, number of pixel groups it was split into)."""
    d = spec.desc(n, c)
    off = _aligned_base(workspace) + int(_lib.load().et_epipolar_forward_workspace_stats_offset(ctypes.byref(d)))
    tiles = n * ((spec.H * spec.W + 31) // 32)
    return workspace[off: off + 4 * tiles].view(torch.int32)


_BWD_EXPLICIT = _lib.ET_VARIANT_BWD_ATOMIC | _lib.ET_VARIANT_BWD_UNSORTED | _lib.ET_VARIANT_NO_TILE


def det_tile_workspace(spec: LayerSpec, n: int, c: int, device) -> torch.Tensor:
    """A caller-owned workspace for backward_nhwc(..., form="tile_det", workspace=...): the forward-layout workspace followed by
    the int64 accumulator (empty tensor if the tile path does not apply)."""
    d = spec.desc(n, c)
    return torch.zeros(int(_lib.load().et_epipolar_backward_tiled_det_workspace_bytes(ctypes.byref(d))), dtype=torch.uint8,
                       device=device)


def _default_backward_form(spec: LayerSpec, tile_bytes: int, use_workspace: bool) -> str:
    """backward_nhwc's choice when the caller names no form (host logic only).  `tile_bytes`: what
    et_epipolar_backward_tiled_workspace_bytes answers for the shape, 0 where the tile path does not apply."""
    if not use_workspace:
        return "atomic"
    form = "tile" if tile_bytes > 0 and not (spec.variant & _BWD_EXPLICIT) else "gather"
    if spec.variant & _lib.ET_VARIANT_BWD_DETERMINISTIC:
        # prefer the deterministic tile form; where it does not apply "gather" is the (bit-reproducible) choice
        form = "tile_det" if form == "tile" and spec.softmax_enabled else "gather"
    return form


def backward_nhwc(spec: LayerSpec, ref, src, cam, grad_out, use_workspace=True, form=None, attn=None, workspace=None,
                  grad_attn=None, ref_index=None, src_index=None):
    """d(feat_ref), d(feat_src) of forward_nhwc.  Four forms of the same gradient:
      "tile"    MFMA tile formulation, d(feat_src) accumulated with float atomics across tiles: fastest,
                reproducible to rounding only (C == 256, K <= 256);
      "tile_det" the same tiles, d(feat_src) accumulated as 64-bit fixed point with integer atomics under a per-pair quantum
                and a tile partition that depends on the inputs only: BIT-REPRODUCIBLE, batch-independent (soft-max on;
                workspace: det_tile_workspace, N H W 256 x 8 bytes beyond the tile form's);
      "gather"  per-(pixel,row) coefficients -> counting sort -> ordered per-row sums: no float atomics, bit-reproducible;
      "atomic"  bilinear-transpose scatter with float atomics (no workspace).
    form=None picks "tile" where it applies (unless the spec's variant names a backward form or NO_TILE) -- "tile_det" when the
    variant carries ET_VARIANT_BWD_DETERMINISTIC and the soft-max is on --, else "gather"; use_workspace=False means "atomic"
    (_default_backward_form).  `attn`: the attention forward_nhwc returned for the same inputs
    (N,K,H,W) -- the tile form then does not recompute the soft-max (one GEMM of five less); the other forms ignore it.
    `workspace`: a caller-owned uint8 tensor for the "tile" / "gather" form instead of the cached one (the tile form's has
    the forward's layout and size: tile_workspace).
    `grad_attn`: d loss / d attn (N,K,H,W) or None -- the gradient through the returned attention, in every form (the *_ga
    entry points: e_k + ga_k in place of e_k = grad_out . S_k in the soft-max gradient).
    `ref_index` / `src_index`: as forward_nhwc's -- ref / src are pools.  The return is then (d ref PER PAIR (N,H,W,C), d src over
    the source POOL (M_src,H,W,C)): the "tile" form adds pair n's rows into map src_index[n] itself
    (et_epipolar_backward_tiled_ix); every other form runs on gathered maps and torch's index_add_ reduces its d(src)."""
    if ref_index is not None or src_index is not None:
        if form is None:        # (the choice backward_nhwc would make for these maps, gathered: it does not depend on N)
            d1 = spec.desc(1, int(ref.shape[-1]))
            form = _default_backward_form(spec, int(_lib.load().et_epipolar_backward_tiled_workspace_bytes(ctypes.byref(d1))),
                                          use_workspace)
        pool_src, given_src = src, src_index
        ref, src, ref_index, src_index = _pair_indices(spec, ref, src, cam, ref_index, src_index, form)
        if given_src is not None and src_index is None:
            # the gathered route: today's call on the pairs' copies, d(src) reduced into the pool
            g_ref, g_pairs = backward_nhwc(spec, ref, src, cam, grad_out, use_workspace, form, attn, workspace, grad_attn)
            idx = device_pair_index(given_src, "src_index", cam.shape[0], pool_src.shape[0], pool_src.device)
            return g_ref, torch.zeros_like(pool_src).index_add_(0, _as_torch_index(idx), g_pairs)
    n, h, w, c = _require_pair(spec, ref, src, cam, ref_index=ref_index, src_index=src_index)
    _require_gpu(grad_out, "grad_out")
    if tuple(grad_out.shape) != (n, h, w, c) or grad_out.device != ref.device:
        raise ValueError("grad_out must be a float32 %s tensor on %s, got %s on %s" %
                         ((n, h, w, c), ref.device, tuple(grad_out.shape), grad_out.device))
    xs, ys, steps = spec.constants(ref.device)
    grad_out = grad_out.contiguous()
    grad_attn = _require_grad_attn(grad_attn, (n, spec.K, h, w), ref.device)
    g_ref = _empty((n, h, w, c), device=ref.device)
    g_src = _empty(None, like=src)
    d = spec.desc(n, c)
    lib = _lib.load()
    tile_bytes = int(lib.et_epipolar_backward_tiled_workspace_bytes(ctypes.byref(d)))
    if form is None:
        form = _default_backward_form(spec, tile_bytes, use_workspace)
    if form not in ("tile", "tile_det", "gather", "atomic"):
        raise ValueError("unknown backward form %r" % (form,))
    args = (ctypes.byref(d), _ptr(xs), _ptr(ys), _ptr(steps), _ptr(cam), _ptr(ref), _ptr(src), _ptr(grad_out), _ptr(grad_attn),
            _ptr(g_ref), _ptr(g_src))
    if form in ("tile", "tile_det"):
        det = form == "tile_det"
        need = int(lib.et_epipolar_backward_tiled_det_workspace_bytes(ctypes.byref(d))) if det else tile_bytes
        if need == 0:
            raise _lib.EpipolarAmdError("the tiled backward needs the 256-channel head (got C=%d, K=%d, %dx%d)" % (c, spec.K, h, w))
        ws = _own_workspace(workspace, need, ref.device, "fwd")
        _last_tile_backward_ws[(ref.device.index, torch.cuda.current_stream(ref.device).cuda_stream)] = weakref.ref(ws)
        if attn is not None:
            _require_f32(attn, "attn", ref.device, (n, spec.K, h, w))
        # (the attention form of the float tile backward is handed the bytes it asked for, the deterministic form all it may use)
        if ref_index is not None or src_index is not None:      # (form "tile": _pair_indices keeps an index for no other)
            _call("et_epipolar_backward_tiled_ix", ref, *args[:7], _ptr(attn), *args[7:], _ptr(ws), ctypes.c_size_t(tile_bytes),
                  _stream(ref), *_ix_args(ref, src, ref_index, src_index))
            return g_ref, g_src
        _call("et_epipolar_backward_tiled_det_ga" if det else "et_epipolar_backward_tiled_ga", ref, *args[:7], _ptr(attn), *args[7:],
              _ptr(ws), ctypes.c_size_t(ws.numel() if det else tile_bytes), _stream(ref))
        if det and POISON_OUTPUTS:          # (test suite: the guard bit surfaces at the call that set it)
            check_tile_errors(workspace=ws)
    else:
        ws, ws_bytes = None, 0
        if form == "gather":
            ws_bytes = int(lib.et_epipolar_backward_workspace_bytes(ctypes.byref(d)))
            ws = _own_workspace(workspace, ws_bytes, ref.device, "bwd")
        _call("et_epipolar_backward_ga", ref, *args, _ptr(ws), ctypes.c_size_t(ws_bytes), _stream(ref))
    return g_ref, g_src


_last_tile_backward_ws = {}     # (device index, stream) -> weak reference to the workspace the last tiled backward ran on


def backward_deferred_tiles(device, header=False, workspace=None):
    """Tiles the most recent tiled backward on `device` (current stream, WHICHEVER host thread launched it: autograd runs the
    backward on a thread of its own) handed from the merged two-array kernel to the one-array kernel because their row set
    exceeds 192 (288) columns -- word 0 of the workspace that call used (or of `workspace`).  Synchronises; a diagnostic
    (tests, profiling).  `header`: the first eight header words, (deferred, error word, four-group tiles met,
    eight-group tiles met early, over-capacity tiles met, ...).  Which tiles
    are deferred depends on the order the blocks of a launch reach them (et_tile_host.h): the count varies from run to run."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    buf = workspace
    if buf is None:
        ref = _last_tile_backward_ws.get((idx, torch.cuda.current_stream(dev).cuda_stream))
        buf = ref() if ref is not None else None
    if buf is None:
        return (0,) * _HEADER_DIAGNOSTICS if header else 0
    words = _header(buf)[:_HEADER_DIAGNOSTICS].tolist()
    return tuple(words) if header else words[_HEADER_DEFERRED]


def atomic_probe(device, rows: int = 1 << 18, blocks: int = 2048, iters: int = 256, reps: int = 5) -> dict:
    """Float-atomic request rate of this box (et_debug_atomic_probe: the access pattern of the tiled backward's d(feat_src)
    accumulation -- one buffer_atomic_fadd_f32 wave-instruction = two 128-byte runs in two pixel rows -- on pseudo-random rows of
    a (rows, 256) fp32 array, 1 GB by default, nothing else in the kernel).  A diagnostic for bench.py: synchronises."""
    dev = torch.device(device)
    dst = torch.zeros(rows, 256, device=dev)
    ms = []
    with torch.cuda.device(dev):
        for r in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _call("et_debug_atomic_probe", None, _ptr(dst), rows, blocks, iters, _stream(dst))
            b.record()
            torch.cuda.synchronize(dev)
            if r:
                ms.append(a.elapsed_time(b))
    ms.sort()
    n_instr = blocks * 4 * iters
    return {"array_MB": rows * 1024 / 1e6, "wave_instructions": n_instr, "ms_min": ms[0], "ms_p50": ms[len(ms) // 2], "ms_max": ms[-1],
            "G_wave_atomics_per_s": n_instr / (ms[len(ms) // 2] * 1e-3) / 1e9, "GB_per_s": n_instr * 256 / (ms[len(ms) // 2] * 1e-3) / 1e9}


def residual_epilogue(feat, out, y=None, scale=None, shift=None, want_finalout=True, want_x=True):
    """All (N,H,W,C) contiguous.  finalout = out + y*scale + shift ; x = feat + finalout."""
    _require_f32(out, "out", out.device)
    n, h, w, c = out.shape
    for t, nm, size in ((feat, "feat", out.numel()), (y, "y", out.numel()), (scale, "scale", c), (shift, "shift", c)):
        if t is not None:       # (feat / y: out's rows in any shape)
            _require_vector(t, nm, size, out.device)
    fin = _empty(None, like=out) if want_finalout else None
    x = _empty(None, like=out) if want_x else None
    _call("et_residual_epilogue", out, n * h * w, c, _ptr(feat), _ptr(out), _ptr(y), _ptr(scale), _ptr(shift), _ptr(fin), _ptr(x),
          _stream(out))
    return fin, x


def residual_gemm_pack(wf: torch.Tensor) -> torch.Tensor:
    """Lay the folded (256 out, 256 in) fp32 weight of the z branch out for `residual_gemm` (split fp16 MFMA fragments +
    the scale).  Returns the packed uint8 buffer; repack when the weights change."""
    _require_gpu(wf, "wf")
    if tuple(wf.shape) != (256, 256):
        raise ValueError("residual_gemm is written for the 256-channel head")
    wf = wf.contiguous()
    packed = torch.empty(int(_lib.load().et_residual_gemm_packed_bytes()), dtype=torch.uint8, device=wf.device)
    _call("et_residual_gemm_pack", wf, _ptr(wf), _ptr(packed), _stream(wf))
    return packed


def _require_packed(packed: torch.Tensor, name: str, device):
    _require_bytes(packed, name, int(_lib.load().et_residual_gemm_packed_bytes()), device,
                   "%s must be the buffer residual_gemm_pack returns" % name)


def residual_gemm(out: torch.Tensor, packed: torch.Tensor, bias: torch.Tensor, feat: torch.Tensor = None) -> torch.Tensor:
    """x = [feat +] bias + out @ Wf^T over the last dimension (256), everything (..., 256) fp32 contiguous: the
    eval-mode `bn(z(out)) [+ out] [+ feat]` (epipolar.py:250-253, resnet.py:388) as one HBM-bound kernel."""
    _require_f32(out, "out", out.device)
    c = out.shape[-1]
    if feat is not None:
        _require_f32(feat, "feat", out.device, out.shape)
    _require_vector(bias, "bias", c, out.device)
    _require_packed(packed, "packed", out.device)
    x = _empty(None, like=out)
    _call("et_residual_gemm", out, out.numel() // c, c, _ptr(out), _ptr(feat), _ptr(packed), _ptr(bias), _ptr(x), _stream(out))
    return x


def z_batch_stats(out: torch.Tensor, packed_wz: torch.Tensor, z_bias: torch.Tensor, workspace: torch.Tensor = None):
    """First pass of the training-mode epilogue (et_z_batch_stats): y = out @ Wz^T + z_bias over the last dimension (256)
    and its per-channel batch mean / biased variance over all rows.  Returns (y, mean, var).  `workspace`: a caller-owned uint8
    tensor instead of the cached one (any contents)."""
    _require_f32(out, "out", out.device, (..., 256), "out must be a contiguous (..., 256) tensor")
    c = out.shape[-1]
    _require_vector(z_bias, "z_bias", c, out.device)
    _require_packed(packed_wz, "packed_wz", out.device)
    rows = out.numel() // c
    y = _empty(None, like=out)
    mean = _empty((c,), device=out.device)
    var = _empty((c,), device=out.device)
    ws_bytes = int(_lib.load().et_z_batch_stats_workspace_bytes(rows))
    ws = _own_workspace(workspace, ws_bytes, out.device, "zstats")
    _call("et_z_batch_stats", out, rows, c, _ptr(out), _ptr(packed_wz), _ptr(z_bias), _ptr(y), _ptr(mean), _ptr(var), _ptr(ws),
          ctypes.c_size_t(ws_bytes), _stream(out))
    return y, mean, var


def z_backward(g: torch.Tensor, y: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor, gamma: torch.Tensor,
               packed_wzt: torch.Tensor, zresidual: bool, workspace: torch.Tensor = None):
    """Backward of the training-mode epilogue w.r.t. `out` and the batch norm's affine parameters (et_z_backward): g, y
    (..., 256) contiguous.  Returns (grad_out, grad_y, grad_gamma, grad_beta).  `workspace`: a caller-owned uint8 tensor instead
    of the cached one (any contents)."""
    _require_f32(g, "g", g.device, (..., 256), "g and y must be contiguous (..., 256) tensors of one shape")
    _require_f32(y, "y", g.device, g.shape, "g and y must be contiguous (..., 256) tensors of one shape")
    c = g.shape[-1]
    for t, nm in ((mean, "mean"), (invstd, "invstd"), (gamma, "gamma")):
        _require_vector(t, nm, c, g.device)
    _require_packed(packed_wzt, "packed_wzt", g.device)
    rows = g.numel() // c
    gout, gy = _empty(None, like=g), _empty(None, like=g)
    ggamma, gbeta = _empty((c,), device=g.device), _empty((c,), device=g.device)
    ws_bytes = int(_lib.load().et_z_backward_workspace_bytes(rows))
    ws = _own_workspace(workspace, ws_bytes, g.device, "zbwd")
    _call("et_z_backward", g, rows, c, _ptr(g), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(gamma), _ptr(packed_wzt),
          1 if zresidual else 0, _ptr(gout), _ptr(gy), _ptr(ggamma), _ptr(gbeta), _ptr(ws), ctypes.c_size_t(ws_bytes), _stream(g))
    return gout, gy, ggamma, gbeta


def z_wgrad(grad_y: torch.Tensor, out: torch.Tensor, workspace: torch.Tensor = None):
    """d Wz (256, 256) = grad_y^T @ out and d bz (256) = grad_y.sum(rows) over (..., 256) contiguous tensors (et_z_wgrad:
    three-term bf16 MFMAs with fp32 accumulation, no atomics, bit-reproducible).  `workspace`: a caller-owned uint8 tensor
    instead of the cached one (any contents)."""
    _require_f32(grad_y, "grad_y", grad_y.device, (..., 256), "grad_y and out must be contiguous (..., 256) tensors of one shape")
    _require_f32(out, "out", grad_y.device, grad_y.shape, "grad_y and out must be contiguous (..., 256) tensors of one shape")
    c = out.shape[-1]
    rows = out.numel() // c
    gw, gb = _empty((c, c), device=out.device), _empty((c,), device=out.device)
    with torch.cuda.device(out.device):
        ws_bytes = int(_lib.load().et_z_wgrad_workspace_bytes(rows))     # (sized by the CU count of the CURRENT device: inside the guard)
        ws = _own_workspace(workspace, ws_bytes, out.device, "zwgrad")
        _call("et_z_wgrad", None, rows, c, _ptr(grad_y), _ptr(out), _ptr(gw), _ptr(gb), _ptr(ws), ctypes.c_size_t(ws_bytes),
              _stream(out))
    return gw, gb


def _require_meta_rows(t: torch.Tensor, name: str, device, shape=None):
    """`t`: the channels-last rows of N pairs, (N, ..., 256) contiguous float32 -- of `shape` where one is given."""
    _require_f32(t, name, device, (..., 256) if shape is None else shape,
                 "%s must be a contiguous channels-last (N, ..., 256) float32 tensor%s on %s, got %s on %s" % (
                     name, "" if shape is None else " of shape %s" % (tuple(shape),), device, tuple(t.shape), t.device))
    if t.dim() < 3 or t.numel() == 0:
        raise ValueError("%s must be (N, ..., 256) with N >= 1 pairs of at least one row, got %s" % (name, tuple(t.shape)))


def meta_pack(weight: torch.Tensor, share: torch.Tensor = None, transpose: bool = False) -> torch.Tensor:
    """Lay `weight[n] + share` (its transpose with `transpose`) out for `meta_gemm`, pair by pair (et_meta_pack): weight N x 65536
    values -- (N, 256 out, 256 in) in any shape --, share 65536 values or None.  Returns the packed uint8 buffer,
    et_residual_gemm_packed_bytes() bytes per pair; repack when the weights change."""
    _require_f32(weight, "weight", weight.device)
    n = weight.shape[0] if weight.dim() else 0
    if n < 1 or weight.numel() != n * 65536:
        raise ValueError("meta_pack is written for the 256-channel head: weight must hold N x 256 x 256 values, got %s" % (tuple(weight.shape),))
    if share is not None:
        _require_vector(share, "share", 65536, weight.device)
    packed = torch.empty(n * int(_lib.load().et_residual_gemm_packed_bytes()), dtype=torch.uint8, device=weight.device)
    _call("et_meta_pack", weight, n, 256, _ptr(weight), _ptr(share), 1 if transpose else 0, _ptr(packed), _stream(weight))
    return packed


def meta_gemm(src: torch.Tensor, packed: torch.Tensor, bias: torch.Tensor = None, feat: torch.Tensor = None) -> torch.Tensor:
    """x[n] = [feat[n] +] [bias +] src[n] @ W_n^T over the rows of every pair n (et_meta_gemm): src (N, ..., 256) channels-last,
    `packed` from `meta_pack` for the same N."""
    _require_meta_rows(src, "src", src.device)
    n, c = src.shape[0], src.shape[-1]
    if feat is not None:
        _require_meta_rows(feat, "feat", src.device, src.shape)
    if bias is not None:
        _require_vector(bias, "bias", c, src.device)
    _require_bytes(packed, "packed", n * int(_lib.load().et_residual_gemm_packed_bytes()), src.device,
                   "packed must be the buffer meta_pack returns for these %d pairs" % n)
    x = _empty(None, like=src)
    _call("et_meta_gemm", src, n, src.numel() // (n * c), c, _ptr(src), _ptr(feat), _ptr(packed), _ptr(bias), _ptr(x), _stream(src))
    return x


def meta_wgrad(g: torch.Tensor, src: torch.Tensor, want_bias: bool = True, workspace: torch.Tensor = None):
    """grad_w (N, 256, 256): grad_w[n] = g[n]^T @ src[n], and grad_b (256) = g summed over every row of every pair (None without
    `want_bias`), from (N, ..., 256) channels-last tensors (et_meta_wgrad: three-term bf16 MFMAs, no atomics, bit-reproducible).
    `workspace`: a caller-owned uint8 tensor instead of the cached one (any contents)."""
    _require_meta_rows(g, "g", g.device)
    _require_meta_rows(src, "src", g.device, g.shape)
    n, c = g.shape[0], g.shape[-1]
    hw = g.numel() // (n * c)
    gw = _empty((n, c, c), device=g.device)
    gb = _empty((c,), device=g.device) if want_bias else None
    ws_bytes = int(_lib.load().et_meta_wgrad_workspace_bytes(n, hw))
    ws = _own_workspace(workspace, ws_bytes, g.device, "metawgrad")
    _call("et_meta_wgrad", g, n, hw, c, _ptr(g), _ptr(src), _ptr(gw), _ptr(gb), _ptr(ws), ctypes.c_size_t(ws_bytes), _stream(g))
    return gw, gb


class MetaFuse(torch.autograd.Function):
    """x = [feat +] share_bias + src . (weight + share_weight)^T per pair: one pack + one GEMM forward; backward a transposed pack +
    the GEMM for d src, et_meta_wgrad for d weight (d share_weight is its sum over the pairs, d share_bias its row sum), d feat = g."""

    @staticmethod
    def forward(ctx, src, weight, share_weight, share_bias, feat):
        ctx.save_for_backward(src, weight, share_weight)
        ctx.has_bias = share_bias is not None
        return meta_gemm(src, meta_pack(weight, share_weight), share_bias, feat)

    @staticmethod
    def backward(ctx, g):
        src, weight, share_weight = ctx.saved_tensors
        need_src, need_w, need_sw, need_b, need_feat = ctx.needs_input_grad
        g = g.contiguous()
        d_src = meta_gemm(g, meta_pack(weight, share_weight, transpose=True)) if need_src else None
        d_w = d_sw = d_b = None
        if need_w or need_sw or (need_b and ctx.has_bias):
            gw, d_b = meta_wgrad(g, src, want_bias=need_b and ctx.has_bias)
            d_w = gw.view_as(weight) if need_w else None
            d_sw = gw.sum(0).view_as(share_weight) if need_sw else None
        return d_src, d_w, d_sw, d_b, g if need_feat else None


def meta_fuse(src: torch.Tensor, weight: torch.Tensor, share_weight: torch.Tensor, share_bias: torch.Tensor = None,
              feat: torch.Tensor = None) -> torch.Tensor:
    """The Meta fusion layer's data pass (modeling/layers/meta.py:42-50 and the hourglass caller's `ret + feat`) for the 256-channel
    head, differentiable in every argument:
        x[n, m, :] = [feat[n, m, :] +] [share_bias +] src[n, m, :] @ (weight[n] + share_weight)^T
    src / feat: (N, ..., 256) channels-last contiguous; weight: N x 256 x 256 values (out, in); share_weight: 256 x 256 values (a
    1x1 convolution's weight as it stands) or None; share_bias (256) or None."""
    _require_meta_rows(src, "src", src.device)
    weight = weight.contiguous()
    if share_weight is not None:
        share_weight = share_weight.contiguous()
    if share_bias is not None:
        share_bias = share_bias.contiguous()
    return MetaFuse.apply(src, weight, share_weight, share_bias, feat)


def _heatmap_peaks(hm: torch.Tensor, radius: float, downsample: float, threshold: float, legacy: int):
    n, j, h, w = hm.shape
    locs = _empty((n, j, 2), device=hm.device)
    scores = _empty((n, j), device=hm.device)
    _call("et_heatmap_peaks", hm, n * j, h, w, _ptr(hm), radius, downsample, threshold, legacy, _ptr(locs), _ptr(scores), _stream(hm))
    return locs, scores


class HeatmapPeaks(torch.autograd.Function):
    """et_heatmap_peaks / et_heatmap_peaks_bwd.  Only the maps receive a gradient; an output nobody differentiated reaches the
    library as NULL (its gradient is not materialised)."""

    @staticmethod
    def forward(ctx, hm, radius, downsample, threshold, legacy):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(hm)
        ctx.call = (radius, downsample, threshold, legacy)
        return _heatmap_peaks(hm, radius, downsample, threshold, legacy)

    @staticmethod
    def backward(ctx, grad_locs, grad_scores):
        hm, = ctx.saved_tensors
        if grad_locs is None and grad_scores is None:
            return None, None, None, None, None
        n, j, h, w = hm.shape
        if grad_locs is not None:
            grad_locs = grad_locs.to(torch.float32).contiguous()
            _require_f32(grad_locs, "grad_locs", hm.device, (n, j, 2))
        if grad_scores is not None:
            grad_scores = grad_scores.to(torch.float32).contiguous()
            _require_f32(grad_scores, "grad_scores", hm.device, (n, j))
        grad = _empty(None, like=hm)
        _call("et_heatmap_peaks_bwd", hm, n * j, h, w, _ptr(hm), *ctx.call, _ptr(grad_locs), _ptr(grad_scores), _ptr(grad), _stream(hm))
        return grad, None, None, None, None


def heatmap_peaks(heatmaps: torch.Tensor, radius: float, downsample: float, threshold: float = 1e-6,
                  legacy_floor_division: bool = False, with_grad: bool = False):
    """find_tensor_peak_batch for a whole batch in ONE kernel: heatmaps (N,J,H,W) -> locations (N,J,2) in image
    coordinates and scores (N,J).
    `with_grad` False (the default): both are detached.  True, and `heatmaps` requires a gradient: locations and scores are
    differentiable in the maps as the reference's are (HeatmapPeaks: et_heatmap_peaks_bwd, one launch, no atomics, the same bits
    from run to run and in any batch); index_w, index_h and the window's box are constants, as the reference takes .data of
    them.  `radius`, `downsample` and `threshold` receive no gradient."""
    _require_gpu(heatmaps, "heatmaps")
    args = (float(radius), float(downsample), float(threshold), int(bool(legacy_floor_division)))
    if with_grad and heatmaps.requires_grad and torch.is_grad_enabled():
        return HeatmapPeaks.apply(heatmaps.contiguous(), *args)
    return _heatmap_peaks(heatmaps.detach().contiguous(), *args)


def _triangulate_bwd(pts, krt, other_krt, corr_pos, downsample: float, resize: float, info, grad_out):
    """et_triangulate_bwd: the (F,V,J,2) float32 gradient in `pts` of either lifting (other_krt / corr_pos None: the views')."""
    f, v, j, _ = pts.shape
    h, w = (0, 0) if corr_pos is None else corr_pos.shape[2:4]
    grad_out = grad_out.to(torch.float64).contiguous()
    _require_gpu(grad_out, "grad_out", torch.float64)
    if tuple(grad_out.shape) != (f, j, 3) or grad_out.device != pts.device:
        raise ValueError("grad_out must be (%d,%d,3) on %s, got %s on %s" % (f, j, pts.device, tuple(grad_out.shape), grad_out.device))
    grad = _empty(None, like=pts)
    _call("et_triangulate_bwd", pts, f, v, j, h, w, _ptr(pts), _ptr(krt), _ptr(other_krt), _ptr(corr_pos), float(downsample),
          float(resize), _ptr(info), _ptr(grad_out), _ptr(grad), _stream(pts))
    return grad


def _triangulate_epipolar(pts, conf, krt, other_krt, corr_pos, downsample, resize, conf_thres, ransac_thres, dlt, want_info):
    f, v, j, _ = pts.shape
    h, w = corr_pos.shape[2:4]
    out = _empty((f, j, 3), device=pts.device, dtype=torch.float64)
    info = torch.empty((f, j), dtype=torch.int32, device=pts.device) if want_info else None
    _call("et_triangulate_epipolar", pts, f, v, j, h, w, _ptr(pts), _ptr(conf), _ptr(krt), _ptr(other_krt), _ptr(corr_pos),
          downsample, resize, conf_thres, ransac_thres, dlt, _ptr(out), _ptr(info), _stream(pts))
    return out, info


class TriangulateEpipolar(torch.autograd.Function):
    """et_triangulate_epipolar / et_triangulate_bwd.  Only the detections receive a gradient: the selection by the scores is
    discrete, and the projections and corr_pos are constants.  The info word is all the backward needs of the forward."""

    @staticmethod
    def forward(ctx, pts, conf, krt, other_krt, corr_pos, *call):
        ctx.set_materialize_grads(False)
        out, info = _triangulate_epipolar(pts, conf, krt, other_krt, corr_pos, *call, True)
        ctx.save_for_backward(pts, krt, other_krt, corr_pos, info)
        ctx.call = call[:2]
        ctx.mark_non_differentiable(info)
        return out, info

    @staticmethod
    def backward(ctx, grad_out, _):
        if grad_out is None:
            return (None,) * 10
        pts, krt, other_krt, corr_pos, info = ctx.saved_tensors
        return (_triangulate_bwd(pts, krt, other_krt, corr_pos, *ctx.call, info, grad_out),) + (None,) * 9


def triangulate_epipolar(pts: torch.Tensor, conf: torch.Tensor, krt: torch.Tensor, other_krt: torch.Tensor,
                         corr_pos: torch.Tensor, *, downsample: float, resize: float, conf_thres: float, ransac_thres: float,
                         dlt: bool = False, want_info: bool = False, with_grad: bool = False):
    """KEYPOINT.TRIANGULATION epipolar (`dlt` False) / epipolar_dlt (True): triangulate_epipolar of
    vision/triangulation.py:234-348 for all frames and joints in ONE kernel (et_triangulate_epipolar, float64 arithmetic).
    pts (F,V,J,2): image coordinates already multiplied by `resize` = IMAGE_RESIZE * PREDICT_RESIZE; conf (F,V,J); krt,
    other_krt (F,V,3,4): every view's projection and its source view's; corr_pos (F,V,H,W,2): the layer's correspondences
    for the frame-major batch.  Returns the (F,J,3) float64 world points -- and, with `want_info`, the (F,J) int32 decision
    word of include/epipolar_amd.h (selected views, views used, branch, no-inlier and clamp flags).

    Two deviations from the reference.  The pair hypotheses are always enumerated: the reference draws 100 random pairs when
    J >= 10 (triangulation.py:303, 322-340), which for V <= 8 is the same hypothesis set in an order that only decides ties;
    this is its own J < 10 branch, deterministic.  A detection whose feature-map pixel lies outside corr_pos is clamped into
    the map and flagged (info bit 19); the reference wraps a negative index and raises on a large one.

    `with_grad` False (the default): the points are detached.  True, and `pts` requires a gradient: the points are differentiable
    in `pts` (TriangulateEpipolar: et_triangulate_bwd, one launch, no atomics, the same bits from run to run and in any batch).
    The backward replays the DLT that the info word names -- the pair, the inliers, the selection, or the one view with its
    correspondence -- with the decision and the correspondence held constant; views that were not used and joints without a
    point receive exactly 0.  conf, the projections and corr_pos receive no gradient.  A vanishing gap between the two smallest
    singular values is not guarded: the gradient is then what float64 autograd through torch.linalg.svd gives as well."""
    _require_gpu(pts, "pts")
    if pts.dim() != 4 or pts.shape[-1] != 2:
        raise ValueError("pts must be (F,V,J,2), got %s" % (tuple(pts.shape),))
    f, v, j, _ = pts.shape
    dev = pts.device
    _require_f32(pts, "pts", dev)
    _require_f32(conf, "conf", dev, (f, v, j))
    _require_f32(krt, "krt", dev, (f, v, 3, 4))
    _require_f32(other_krt, "other_krt", dev, (f, v, 3, 4))
    _require_gpu(corr_pos, "corr_pos")
    if corr_pos.dim() != 5:
        raise ValueError("corr_pos must be (F,V,H,W,2) = (%d,%d,H,W,2), got %s" % (f, v, tuple(corr_pos.shape)))
    h, w = corr_pos.shape[2:4]
    _require_f32(corr_pos, "corr_pos", dev, (f, v, h, w, 2))
    call = (float(downsample), float(resize), float(conf_thres), float(ransac_thres), int(bool(dlt)))
    if with_grad and pts.requires_grad and torch.is_grad_enabled():
        out, info = TriangulateEpipolar.apply(pts, conf.detach(), krt.detach(), other_krt.detach(), corr_pos.detach(), *call)
    else:
        out, info = _triangulate_epipolar(pts, conf, krt, other_krt, corr_pos, *call, want_info)
    return (out, info) if want_info else out


VIEW_METHODS = {"pymvg": 0, "naive": 1, "refine": 2}


def _triangulate_views(pts, conf, krt, method, conf_thres, ransac_thres, want_info):
    f, v, j, _ = pts.shape
    out = _empty((f, j, 3), device=pts.device, dtype=torch.float64)
    info = torch.empty((f, j), dtype=torch.int32, device=pts.device) if want_info else None
    _call("et_triangulate_views", pts, f, v, j, _ptr(pts), _ptr(conf), _ptr(krt), method, conf_thres, ransac_thres, _ptr(out),
          _ptr(info), _stream(pts))
    return out, info


class TriangulateViews(torch.autograd.Function):
    """et_triangulate_views / et_triangulate_bwd.  Only the detections receive a gradient (TriangulateEpipolar)."""

    @staticmethod
    def forward(ctx, pts, conf, krt, *call):
        ctx.set_materialize_grads(False)
        out, info = _triangulate_views(pts, conf, krt, *call, True)
        ctx.save_for_backward(pts, krt, info)
        ctx.mark_non_differentiable(info)
        return out, info

    @staticmethod
    def backward(ctx, grad_out, _):
        if grad_out is None:
            return (None,) * 6
        pts, krt, info = ctx.saved_tensors
        return (_triangulate_bwd(pts, krt, None, None, 0.0, 0.0, info, grad_out),) + (None,) * 5


def triangulate_views(pts: torch.Tensor, conf: torch.Tensor, krt: torch.Tensor, *, method: str, conf_thres: float,
                      ransac_thres: float = 3.0, want_info: bool = False, with_grad: bool = False):
    """KEYPOINT.TRIANGULATION pymvg / naive / refine (vision/triangulation.py:425-441, 99-154, 162-232) for all frames and joints
    in ONE kernel (et_triangulate_views, float64 arithmetic): the liftings that need only detections, scores and projections.
    pts (F,V,J,2): image coordinates; conf (F,V,J); krt (F,V,3,4).  `pymvg`: the DLT over the views above `conf_thres`, the
    threshold lowered in steps of 0.05 until two views remain (`ransac_thres` is not read).  `naive`: every pair of views above
    `conf_thres` is a hypothesis, the first with the most rays within `ransac_thres` of its two-view point wins and that point is
    returned.  `refine`: the same search, then the DLT over the winner's inliers when it has more than one.  Returns the (F,J,3)
    float64 world points -- and, with `want_info`, the (F,J) int32 decision word of include/epipolar_amd.h (views selected, views
    used, zeros written, threshold steps).  A joint with fewer than two usable views, or no inlier, is (0, 0, 0) and flagged.

    One deviation from the reference, the one `triangulate_epipolar` states: the pair hypotheses of `naive` / `refine` are always
    enumerated.  The reference draws 100 random ordered pairs per joint; for V <= 8 "all ordered pairs in lexicographic order,
    cyclically" is one sequence those draws can produce, it visits every pair, and its result is the result of the enumeration
    (tests/golden/make_triangulation_ransac_golden.py runs the reference on exactly that sequence).

    `with_grad` False (the default): the points are detached.  True, and `pts` requires a gradient: the points are differentiable
    in `pts` (TriangulateViews: et_triangulate_bwd, one launch, no atomics, the same bits from run to run and in any batch) --
    the gradient of the DLT over the views the info word names (pymvg's selection, naive's winning pair, refine's inliers), the
    decision held constant; views that were not used and flagged joints receive exactly 0, conf and krt no gradient.  A
    vanishing gap between the two smallest singular values is not guarded: the gradient is then what float64 autograd through
    torch.linalg.svd gives as well."""
    if method not in VIEW_METHODS:
        raise ValueError("method must be one of %s, got %r" % (", ".join(VIEW_METHODS), method))
    _require_gpu(pts, "pts")
    if pts.dim() != 4 or pts.shape[-1] != 2:
        raise ValueError("pts must be (F,V,J,2), got %s" % (tuple(pts.shape),))
    f, v, j, _ = pts.shape
    dev = pts.device
    _require_f32(pts, "pts", dev)
    _require_f32(conf, "conf", dev, (f, v, j))
    _require_f32(krt, "krt", dev, (f, v, 3, 4))
    call = (VIEW_METHODS[method], float(conf_thres), float(ransac_thres))
    if with_grad and pts.requires_grad and torch.is_grad_enabled():
        out, info = TriangulateViews.apply(pts, conf.detach(), krt.detach(), *call)
    else:
        out, info = _triangulate_views(pts, conf, krt, *call, want_info)
    return (out, info) if want_info else out


def _optional_vis(vis, shape, device):
    if vis is not None:
        _require_f32(vis, "vis", device, shape)
    return vis


def eval_jdr(pred: torch.Tensor, target: torch.Tensor, thr: float = 0.5, want_xy: bool = False):
    """JDR (modeling/metrics/metrics2d.py:294-324, hm_type 'gaussian') of predicted against target heat maps, both (N,J,H,W)
    float32, on the device (et_eval_jdr: one block per map finds both first maxima, a second small launch counts).  Returns
    `dists` (J,N) float64 -- the reference's layout: -1 where the target's maximum lies at x <= 1 or y <= 1, else the norm of
    (pred - target) / (H/10, W/10), x over the HEIGHT term as the reference has it -- and `acc` (J+1,) float64: acc[1 + j] the
    share of joint j's counted distances below `thr` (-1: none counts), acc[0] their average in joint order (NaN when no joint
    counts; the reference raises there).  With `want_xy` also get_max_preds' masked integer coordinates of both stacks,
    (N,J,2) float32.  Bit-equal to the reference; no synchronisation.  2 <= H, W and H * W <= 16384.  No gradient."""
    _require_gpu(pred, "pred")
    if pred.dim() != 4:
        raise ValueError("pred must be (N,J,H,W), got %s" % (tuple(pred.shape),))
    n, j, h, w = pred.shape
    dev = pred.device
    _require_f32(pred, "pred", dev)
    _require_f32(target, "target", dev, (n, j, h, w))
    dists = _empty((j, n), device=dev, dtype=torch.float64)
    acc = _empty((j + 1,), device=dev, dtype=torch.float64)
    pred_xy = _empty((n, j, 2), device=dev) if want_xy else None
    target_xy = _empty((n, j, 2), device=dev) if want_xy else None
    _call("et_eval_jdr", pred, n, j, h, w, _ptr(pred), _ptr(target), float(thr), _ptr(dists), _ptr(acc), _ptr(pred_xy), _ptr(target_xy),
          _stream(pred))
    return (dists, acc, pred_xy, target_xy) if want_xy else (dists, acc)


_MARKS = {}     # (device, values) -> float64 device array: the thresholds / curve points of eval_pck, filled on the host once


def _marks(values, device) -> torch.Tensor:
    host = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    key = (str(device), host.tobytes())
    if key not in _MARKS:
        _MARKS[key] = torch.from_numpy(host).to(device)
        torch.cuda.current_stream(device).synchronize()      # once per set of values: later calls on any stream find it uploaded
    return _MARKS[key]


def eval_pck(locs: torch.Tensor, gt: torch.Tensor, vis: torch.Tensor = None, *, thresholds=(1, 2, 5, 10, 20, 30, 40, 50, 60, 80, 100),
             max_threshold=20):
    """calculate_err (modeling/metrics/metrics2d.py:199-235; its PCKs are calc_pck's) on the device (et_eval_pck).  locs (N,J,2)
    float32 detections, gt (N,J,2) float64, vis (N,J) float32 or None (all visible; an item counts when vis != 0).  Returns `pck`
    (T,) float64: count(err < th) * 100 / count over the whole batch for every th of `thresholds` (cfg.TEST.THRESHOLDS; NaN when
    nothing counts), `err_joints` (N,M) float64: per sample the count of err < c over the M = int(max_threshold) points c of
    np.linspace(0, max_threshold, num=int(max_threshold)) (cfg.TEST.MAX_TH; made with NumPy, so its bits are the reference's), and
    `total_joints` (N,1) float64.  The error is |x - x_gt| -- x ONLY: the reference's `detected_points[:1, j]` takes the first row
    of its (2,J) array.  Bit-equal to the reference; no synchronisation (the thresholds are uploaded once and kept).  No gradient."""
    _require_gpu(locs, "locs")
    if locs.dim() != 3 or locs.shape[-1] != 2:
        raise ValueError("locs must be (N,J,2), got %s" % (tuple(locs.shape),))
    n, j, _ = locs.shape
    dev = locs.device
    _require_f32(locs, "locs", dev)
    _require_gpu(gt, "gt", torch.float64)
    if gt.device != dev or not gt.is_contiguous() or tuple(gt.shape) != (n, j, 2):
        raise ValueError("gt must be a contiguous float64 tensor of shape %s on %s, got %s on %s" % ((n, j, 2), dev, tuple(gt.shape), gt.device))
    _optional_vis(vis, (n, j), dev)
    th = _marks(thresholds, dev)
    curve = _marks(np.linspace(0, max_threshold, num=int(max_threshold)), dev)
    t, m = th.numel(), curve.numel()
    pck = _empty((t,), device=dev, dtype=torch.float64)
    err_joints = _empty((n, m), device=dev, dtype=torch.float64)
    total_joints = _empty((n, 1), device=dev, dtype=torch.float64)
    _call("et_eval_pck", locs, n, j, _ptr(locs), _ptr(gt), _ptr(vis), t, _ptr(th if t else None), m, _ptr(curve if m else None),
          _ptr(pck if t else None), _ptr(err_joints if m else None), _ptr(total_joints), _stream(locs))
    return pck, err_joints, total_joints


def eval_epe(pred: torch.Tensor, gt: torch.Tensor, vis: torch.Tensor = None, *, unit: float = 1.0, max_dist: float = 150.0):
    """EPEmean (modeling/metrics/metrics3d.py:5-46) in float64 on the device (et_eval_epe).  pred, gt (F,J,3) float64, vis (F,J)
    float32 or None; `unit` and `max_dist` (cfg.TEST.EPEMEAN_MAX_DIST) are host numbers.  err = sqrt((dx^2 + dy^2) + dz^2) * unit,
    replaced by max_dist where it exceeds it.  Returns `mean`, a 0-d float64 tensor -- over all F * J items: visibility does not
    enter it, as in the reference -- summed in a fixed order, and `per_joint` (F,J) float64: err with the items of vis == 0 set
    to 0 (the reference returns row 0 of it), bit-equal to the reference.  No synchronisation.  No gradient."""
    _require_gpu(pred, "pred", torch.float64)
    if pred.dim() != 3 or pred.shape[-1] != 3:
        raise ValueError("pred must be (F,J,3), got %s" % (tuple(pred.shape),))
    f, j, _ = pred.shape
    dev = pred.device
    _require_gpu(gt, "gt", torch.float64)
    for t, name in ((pred, "pred"), (gt, "gt")):
        if t.device != dev or not t.is_contiguous() or tuple(t.shape) != (f, j, 3):
            raise ValueError("%s must be a contiguous float64 tensor of shape %s on %s, got %s on %s" % (
                name, (f, j, 3), dev, tuple(t.shape), t.device))
    _optional_vis(vis, (f, j), dev)
    mean = _empty((), device=dev, dtype=torch.float64)
    per_joint = _empty((f, j), device=dev, dtype=torch.float64)
    _call("et_eval_epe", pred, f, j, _ptr(pred), _ptr(gt), _ptr(vis), float(unit), float(max_dist), _ptr(mean), _ptr(per_joint),
          _stream(pred))
    return mean, per_joint


LOSS_KINDS = {"joint": _lib.ET_LOSS_JOINT, "smoothmse": _lib.ET_LOSS_SMOOTHMSE, "mse": _lib.ET_LOSS_MSE}


def _require_points(points: torch.Tensor, shape, device):
    _require_gpu(points, "points", torch.float64)
    if points.device != device or not points.is_contiguous() or tuple(points.shape) != tuple(shape):
        raise ValueError("points must be a contiguous float64 tensor of shape %s on %s, got %s on %s" % (
            tuple(shape), device, tuple(points.shape), points.device))


def heatmap_targets(points: torch.Tensor, H: int, W: int, sigma: float, downsample: float) -> torch.Tensor:
    """Heatmapcreator.get (data/transforms/keypoints2d.py:3-36) on the device (et_heatmap_targets): points (N,J,2) float64, (u, v) in
    image pixels -> the (N,J,H,W) float32 targets the reference's data loader makes on the CPU, with its arithmetic: float32 grid,
    float64 distance, exp rounded once to float32; v pairs with the rows; no visibility mask; the background is 0.01, not 0.
    H * W <= 16384.  No synchronisation.  No gradient."""
    _require_gpu(points, "points", torch.float64)
    if points.dim() != 3 or points.shape[-1] != 2:
        raise ValueError("points must be (N,J,2), got %s" % (tuple(points.shape),))
    n, j, _ = points.shape
    _require_points(points, (n, j, 2), points.device)
    out = _empty((n, j, int(H), int(W)), device=points.device)
    _call("et_heatmap_targets", points, n, j, int(H), int(W), _ptr(points), float(sigma), float(downsample), _ptr(out), _stream(points))
    return out


class HeatmapLoss(torch.autograd.Function):
    """et_heatmap_loss / et_heatmap_loss_bwd.  Only `pred` receives a gradient; grad_output and the denominator stay on the
    device."""

    @staticmethod
    def forward(ctx, pred, target, points, weight, kind, per_joint, sigma, downsample):
        n, j, h, w = pred.shape
        dev = pred.device
        partials = _empty((n * j,), device=dev, dtype=torch.float64)
        loss = _empty((), device=dev)
        den = _empty((), device=dev, dtype=torch.float64)
        _call("et_heatmap_loss", pred, kind, n, j, h, w, _ptr(pred), _ptr(target), _ptr(points), sigma, downsample, _ptr(weight),
              int(per_joint), _ptr(partials), _ptr(loss), _ptr(den), _stream(pred))
        ctx.save_for_backward(pred, target, points, weight, den)
        ctx.call = (kind, sigma, downsample)
        return loss

    @staticmethod
    def backward(ctx, grad_out):
        pred, target, points, weight, den = ctx.saved_tensors
        kind, sigma, downsample = ctx.call
        n, j, h, w = pred.shape
        go = grad_out.to(pred.device, torch.float32).reshape(1).contiguous()
        grad = _empty(None, like=pred)
        _call("et_heatmap_loss_bwd", pred, kind, n, j, h, w, _ptr(pred), _ptr(target), _ptr(points), sigma, downsample, _ptr(weight),
              _ptr(den), _ptr(go), _ptr(grad), _stream(pred))
        return grad, None, None, None, None, None, None, None


def heatmap_loss(pred: torch.Tensor, target: torch.Tensor = None, weight: torch.Tensor = None, *, kind: str, per_joint: bool = False,
                 points: torch.Tensor = None, sigma: float = None, downsample: float = None) -> torch.Tensor:
    """The criterion KEYPOINT.LOSS names (modeling/model.py:59-71) of pred (N,J,H,W) float32 as a float32 scalar on the device, with
    its gradient for `pred` (et_heatmap_loss / et_heatmap_loss_bwd: one pass over the maps each way, float64 sums in a fixed order,
    no atomics, no synchronisation).  `kind`:
      joint       JointsMSELoss (metrics2d.py:18-41): per joint the mean of (pred * w - gt * w) ** 2 over batch and pixels, summed over
                  the joints and divided by J unless `per_joint`;
      smoothmse   KeypointsMSESmoothLoss (:43-58): t = (gt - pred) ** 2 * w, replaced by t ** 0.1 * 400 ** 0.9 where t > 400, summed
                  and divided by H * W * max(1, sum(w)); w carries no gradient;
      mse         MaskedMSELoss with masks=None (:61-81): the mean of (pred - gt) ** 2; `weight` must be None.
    The target is EITHER `target` (N,J,H,W) float32 OR `points` (N,J,2) float64 with `sigma` and `downsample`: then every lane makes
    the target of its own pixels as heatmap_targets does and no dense target is read or written.  `weight`: (N,J) or (N,J,1) float32,
    None = ones.  A `pred` that is not contiguous (the head of a channels-last trunk) is copied once; target, points and weight
    must be contiguous.  H * W <= 16384."""
    if kind not in LOSS_KINDS:
        raise ValueError("kind must be one of %s, got %r" % (", ".join(LOSS_KINDS), kind))
    if (target is None) == (points is None):
        raise ValueError("give either target or points (with sigma and downsample), not %s" % ("neither" if target is None else "both"))
    if kind == "mse" and weight is not None:
        raise ValueError("kind 'mse' takes no weight (MaskedMSELoss with masks=None)")
    _require_gpu(pred, "pred")
    if pred.dim() != 4:
        raise ValueError("pred must be (N,J,H,W), got %s" % (tuple(pred.shape),))
    n, j, h, w = pred.shape
    dev = pred.device
    if target is not None:
        _require_f32(target, "target", dev, (n, j, h, w))
        sigma = downsample = 0.0
    else:
        if sigma is None or downsample is None:
            raise ValueError("points need sigma and downsample")
        _require_points(points, (n, j, 2), dev)
    if weight is not None:
        _require_gpu(weight, "weight")
        if tuple(weight.shape) not in ((n, j), (n, j, 1)):
            raise ValueError("weight must be (N,J) or (N,J,1) = (%d,%d[,1]), got %s" % (n, j, tuple(weight.shape)))
        _require_f32(weight, "weight", dev)
    return HeatmapLoss.apply(pred.contiguous(), target, points, weight, LOSS_KINDS[kind], bool(per_joint), float(sigma), float(downsample))


def rpsm_workspace_bytes(frames: int, joints: int, first_nbins: int, recur_nbins: int) -> int:
    return int(_lib.load().et_rpsm_workspace_bytes(int(frames), int(joints), int(first_nbins), int(recur_nbins)))


def rpsm(heatmaps: torch.Tensor, cams: torch.Tensor, trans: torch.Tensor, center: torch.Tensor, limb_length: torch.Tensor, *,
         first_limb_length: torch.Tensor = None, parent=None, image_size, grid_size: float, first_nbins: int, recur_nbins: int,
         recur_depth: int, tolerance: float, align_corners: bool = False, want_path: bool = False, workspace: torch.Tensor = None):
    """KEYPOINT.TRIANGULATION rpsm: the recursive pictorial structure model of modeling/pictorial_cuda.py:222-254 for all frames
    in three kinds of HIP kernel (et_rpsm: unary, one max-product launch per tree level, one block per frame for the back-track and
    the RECUR_DEPTH levels), float32 as the reference.  heatmaps (F,V,J,H,W); cams (F,V,3,4): projections to image pixels (the
    reference's origK @ RT); trans (F,V,2,3): the crop transforms (pictorial.crop_transform); center (F,3): the first grid's centre;
    limb_length (F,E) or (E,), E = J - 1: limb e ends at the e-th non-root joint in ascending order; first_limb_length: the first
    stage's lengths (None: limb_length); parent: J entries, the root has -1 (None: the H36M skeleton, pictorial.H36M_PARENT);
    image_size (w, h) = DATASETS.IMAGE_SIZE.  Returns the (F,J,3) float32 pose -- and, with `want_path`, the (F,1+recur_depth,J)
    int32 bins chosen at every level.  `workspace`: a uint8 buffer of at least rpsm_workspace_bytes(...) bytes, any alignment (None:
    allocated here).

    One deviation from the reference: limb compatibility is the band | ||x_a - x_c + 1e-6|| + 1e-9 - L | < tolerance computed from
    the bin positions, which is what the reference's own compute_pairwise builds for the recursion levels; its first stage reads a
    precomputed 0/1 table (PICT_STRUCT.PAIRWISE_FILE) instead, and a table that is not such a band cannot be expressed.
    No gradient."""
    _require_gpu(heatmaps, "heatmaps")
    if heatmaps.dim() != 5:
        raise ValueError("heatmaps must be (F,V,J,H,W), got %s" % (tuple(heatmaps.shape),))
    f, v, j, h, w = heatmaps.shape
    dev = heatmaps.device
    _require_f32(heatmaps, "heatmaps", dev)
    _require_f32(cams, "cams", dev, (f, v, 3, 4))
    _require_f32(trans, "trans", dev, (f, v, 2, 3))
    _require_f32(center, "center", dev, (f, 3))

    def limbs(t, name):
        _require_gpu(t, name)
        if tuple(t.shape) == (j - 1,):
            t = t.expand(f, j - 1).contiguous()
        _require_f32(t, name, dev, (f, j - 1), "%s must be a contiguous float32 tensor of shape %s or %s on %s, got %s on %s" % (
            name, (f, j - 1), (j - 1,), dev, tuple(t.shape), t.device))
        return t

    limb_length = limbs(limb_length, "limb_length")
    if first_limb_length is not None:
        first_limb_length = limbs(first_limb_length, "first_limb_length")
    if parent is None:
        from .pictorial import H36M_PARENT as parent
    parent = [int(p) for p in parent]
    if len(parent) != j:
        raise ValueError("parent names %d joints, heatmaps have %d" % (len(parent), j))
    parent_c = (ctypes.c_int32 * j)(*parent)
    need = rpsm_workspace_bytes(f, j, first_nbins, recur_nbins)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    else:
        _require_bytes(workspace, "workspace", need, dev)
    out = _empty((f, j, 3), device=dev)
    path = torch.empty((f, 1 + max(int(recur_depth), 0), j), dtype=torch.int32, device=dev) if want_path else None
    _call("et_rpsm", heatmaps, f, v, j, h, w, _ptr(heatmaps), _ptr(cams), _ptr(trans), _ptr(center), _ptr(limb_length),
          _ptr(first_limb_length), parent_c, float(image_size[0]), float(image_size[1]), float(grid_size), int(first_nbins),
          int(recur_nbins), int(recur_depth), float(tolerance), int(bool(align_corners)), _ptr(out), _ptr(path), _ptr(workspace),
          workspace.numel(), _stream(heatmaps))
    return (out, path) if want_path else out


class EpipolarAttend(torch.autograd.Function):
    """out = sum_k softmax_k(scale * mask(f_ref . S_k)) S_k with S_k the K bilinear
    samples of f_src on the pixel's epipolar segment (epipolar.py:188-247).
    Inputs/outputs are logical NCHW; attn and corr_pos are returned without
    gradient (the reference never back-propagates through them in the
    configurations of BASELINE.json) -- unless `attn_grad`: then attn is an ordinary
    differentiable output, as in the reference (epipolar.py:245, 263), and its gradient
    goes into the same HIP backward (backward_nhwc's grad_attn).  The backward takes backward_nhwc's default form: the MFMA tile kernel for
    the 256-channel head (float atomics across tiles, reproducible to rounding; with ET_VARIANT_BWD_DETERMINISTIC in the spec's
    variant -- EPIPOLAR_AMD.DETERMINISTIC -- its bit-reproducible integer-sum form), the bit-reproducible gather form
    otherwise or when the spec's variant carries ET_VARIANT_NO_TILE."""

    @staticmethod
    def forward(ctx, feat_ref, feat_src, cam, spec: LayerSpec, attn_grad: bool = False):
        ref = to_nhwc(feat_ref)
        src = to_nhwc(feat_src)
        out, attn, corr = forward_nhwc(spec, ref, src, cam)
        ctx.spec = spec
        ctx.save_for_backward(ref, src, cam, attn)       # (the soft-max output, as autograd keeps it in the reference)
        _mark_attention(ctx, attn, corr, attn_grad)
        return out.permute(0, 3, 1, 2), attn, corr

    @staticmethod
    def backward(ctx, grad_out, grad_attn, _gc):
        ref, src, cam, attn = ctx.saved_tensors
        g = torch.zeros_like(ref) if grad_out is None else to_nhwc(grad_out)     # (None: attn_grad, a loss on the attention alone)
        g_ref, g_src = backward_nhwc(ctx.spec, ref, src, cam, g, attn=attn, grad_attn=grad_attn if ctx.attn_grad else None)
        need_ref, need_src = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        return (g_ref.permute(0, 3, 1, 2) if need_ref else None,
                g_src.permute(0, 3, 1, 2) if need_src else None, None, None, None)


class EpipolarAttendIndexed(torch.autograd.Function):
    """EpipolarAttend with the pairs named by index into stacks of maps (ET_HAS_PAIR_INDEX): `pool_ref` (M_ref,C,H,W) and
    `pool_src` (M_src,C,H,W), logical NCHW -- they may be ONE tensor --, `cam` (N,27), and `ref_index` / `src_index` as
    forward_nhwc takes them (None: that operand holds one map per pair).  Pair n attends pool_ref[ref_index[n]] to
    pool_src[src_index[n]]; out (N,C,H,W), attn and corr_pos are per pair.  What autograd keeps are the POOLS, never gathered
    copies; d(pool_src) comes straight from the tile kernel (pair n's rows added into map src_index[n]), d(pool_ref) is the
    per-pair d(feat_ref) reduced with index_add_ (with a None ref_index: the kernel's tensor itself); when both pools are one
    tensor autograd sums the two.  Shapes and specs the indexed kernels do not take (pair_index_applies) run on torch-gathered
    maps inside the same calls, with the same results."""

    @staticmethod
    def forward(ctx, pool_ref, pool_src, cam, spec: LayerSpec, ref_index=None, src_index=None, attn_grad: bool = False):
        ref = to_nhwc(pool_ref)
        src = ref if pool_src is pool_ref else to_nhwc(pool_src)
        out, attn, corr = forward_nhwc(spec, ref, src, cam, ref_index=ref_index, src_index=src_index)
        ctx.spec, ctx.index = spec, (ref_index, src_index)
        ctx.save_for_backward(ref, src, cam, attn)
        _mark_attention(ctx, attn, corr, attn_grad)
        return out.permute(0, 3, 1, 2), attn, corr

    @staticmethod
    def backward(ctx, grad_out, grad_attn, _gc):
        ref, src, cam, attn = ctx.saved_tensors
        ref_index, src_index = ctx.index
        n = cam.shape[0]
        g = (torch.zeros((n,) + tuple(ref.shape[1:]), device=ref.device) if grad_out is None else to_nhwc(grad_out))
        g_ref, g_src = backward_nhwc(ctx.spec, ref, src, cam, g, attn=attn, grad_attn=grad_attn if ctx.attn_grad else None,
                                     ref_index=ref_index, src_index=src_index)
        need_ref, need_src = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if need_ref and ref_index is not None:
            idx = device_pair_index(ref_index, "ref_index", n, ref.shape[0], ref.device)
            g_ref = torch.zeros_like(ref).index_add_(0, _as_torch_index(idx), g_ref)
        return (g_ref.permute(0, 3, 1, 2) if need_ref else None,
                g_src.permute(0, 3, 1, 2) if need_src else None, None, None, None, None, None)
