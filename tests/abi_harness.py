"""Helpers of tests/test_gpu_workspace_contracts.py and tests/test_gpu_redzones.py (a plain module: importing it needs no GPU).

  * inputs of a call (camera rig, feature maps) and the tile workspace's header / regions as the host sees them
    (csrc/et_tile_host.h: 64-word header | perm[tiles * 32] | overflow list[tiles] | stats[tiles] | ...);
  * `Arena`: every output tensor and every workspace of ONE call carved out of one allocation, a guard band of GUARD_BYTES
    (one 64 x 256 fp32 tile: a whole mis-addressed tile row lands inside it) of the byte GUARD_BYTE on both sides of each;
  * `frozen` / `assert_unchanged`: the inputs of a call, bit for bit, before and after.
"""
import ctypes

import torch

C = 256
GUARD_BYTES = 64 * 256 * 4
GUARD_BYTE = 0xA5               # neither the NaN poison of the outputs (0xFF) nor a plausible value: -2.87e-16 as a float
HEADER_WORDS = 64
TILE_PIX = 32


def pair_inputs(n, h, w, seed, rig="ring", scale=1.0):
    """ref, src (N,H,W,256) post-ReLU random maps and cam (N,27) of `n` pairs of the rig, on the GPU."""
    from epipolar_transformers_amd import camera, synthetic as syn

    per = 4 if rig in ("ring", "h36m_room") else 2
    P1, P2 = syn.rig_pairs(rig, (n + per - 1) // per, 4 * max(h, w), seed=seed, jitter=(0.05, 8.0))
    g = torch.Generator(device="cuda").manual_seed(seed)
    ref = torch.randn(n, h, w, C, device="cuda", generator=g).relu_() * scale
    src = torch.randn(n, h, w, C, device="cuda", generator=g).relu_() * scale
    return ref, src, camera.pair_algebra(P1[:n], P2[:n]).cuda()


def tiles_of(n, h, w):
    return n * ((h * w + TILE_PIX - 1) // TILE_PIX)


def ws_base(ws):
    """Offset of the first 256-byte boundary inside the workspace: where the library puts the header."""
    return (-ws.data_ptr()) % 256


def ws_header(ws):
    b = ws_base(ws)
    return ws[b:b + 4 * HEADER_WORDS].view(torch.int32)


def ws_overflow(ws):
    return int(ws_header(ws)[0].item())


def ws_overflow_list(ws, n, h, w, count=None):
    """The overflow-tile list region (`tiles` int32 behind perm); the first `count` entries when given."""
    t = tiles_of(n, h, w)
    b = ws_base(ws) + 4 * (HEADER_WORDS + t * TILE_PIX)
    lst = ws[b:b + 4 * t].view(torch.int32)
    return lst if count is None else lst[:count]


def assert_overflow_list_is_sane(ws, n, h, w):
    """count <= tiles, and the first `count` entries are distinct valid tile indices."""
    t, cnt = tiles_of(n, h, w), ws_overflow(ws)
    assert 0 <= cnt <= t, "overflow count %d beyond the %d tiles (and list entries) of the call" % (cnt, t)
    lst = ws_overflow_list(ws, n, h, w, cnt).cpu().tolist()
    assert all(0 <= v < t for v in lst), "the overflow list holds an index that is no tile of the call"
    assert len(set(lst)) == cnt, "a tile appears twice in the overflow list (%d entries, %d distinct)" % (cnt, len(set(lst)))
    return cnt


def bits(t):
    """The tensor's memory as integers: comparisons bit for bit, NaNs included."""
    t = t.contiguous().view(-1)
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def frozen(**tensors):
    """Clones of a call's inputs (None entries are skipped), for assert_unchanged after the call."""
    return {k: (v, v.clone()) for k, v in tensors.items() if v is not None}


def assert_unchanged(snap):
    for name, (now, before) in snap.items():
        assert same_bits(now, before), "the call modified its input `%s`" % name


def fill_bytes(t, how, seed=0):
    """Overwrite a uint8 tensor: "zero", "ff" (NaN as a float, -1 as an int) or "random" bytes."""
    if how == "zero":
        t.zero_()
    elif how == "ff":
        t.fill_(0xFF)
    else:
        assert how == "random", how
        g = torch.Generator(device=t.device).manual_seed(1234 + seed)
        t.copy_(torch.randint(0, 256, (t.numel(),), device=t.device, dtype=torch.uint8, generator=g))
    return t


def dirty_tile_workspace(ws, how, header_value, seed=0):
    """A zeroed tile workspace made to look used: everything behind the 64-word header `how`-filled, header words 0 and 2..9
    (the overflow count and the counters of one call) set to `header_value`; word 1 (the sticky error word) and words
    10..63 (touched by nothing) stay zero."""
    b = ws_base(ws)
    fill_bytes(ws[b + 4 * HEADER_WORDS:], how, seed)
    hdr = ws_header(ws)
    hdr[0] = header_value
    hdr[2:10] = header_value
    return ws


class Arena:
    """Outputs and workspaces of one call, carved out of ONE uint8 allocation:
        guard | item 0 | guard | item 1 | ... | guard,   every guard >= GUARD_BYTES of GUARD_BYTE,
    items 256-byte aligned (+ `shift` bytes), a guard starting at the item's last byte + 1.  Items start as 0xFF bytes (NaN /
    -1) unless `fill` says otherwise.  check() asserts that every guard byte still holds GUARD_BYTE."""

    def __init__(self):
        self._items, self._buf, self._spans = [], None, {}

    def add(self, name, shape, dtype=torch.float32, fill=0xFF, shift=0):
        assert self._buf is None and name not in [i[0] for i in self._items]
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        self._items.append((name, shape, dtype, fill, shift))
        return self

    def build(self, device="cuda"):
        size = lambda shape, dtype: int(torch.tensor([], dtype=dtype).element_size() * int(torch.Size(shape).numel()))
        total = GUARD_BYTES + sum(size(s, d) + 512 + sh + GUARD_BYTES for _, s, d, _, sh in self._items)
        self._buf = torch.full((total,), GUARD_BYTE, dtype=torch.uint8, device=device)
        cur = GUARD_BYTES
        for name, shape, dtype, fill, shift in self._items:
            cur += (-(self._buf.data_ptr() + cur)) % 256 + shift
            nbytes = size(shape, dtype)
            self._spans[name] = (cur, nbytes, shape, dtype)
            self._buf[cur:cur + nbytes] = fill
            cur += nbytes + GUARD_BYTES
        assert cur <= total
        return self

    def __getitem__(self, name):
        start, nbytes, shape, dtype = self._spans[name]
        return self._buf[start:start + nbytes].view(dtype).view(shape)

    def check(self):
        torch.cuda.synchronize()
        guard = torch.ones(self._buf.numel(), dtype=torch.bool, device=self._buf.device)
        for start, nbytes, _, _ in self._spans.values():
            guard[start:start + nbytes] = False
        bad = torch.nonzero(guard & (self._buf != GUARD_BYTE)).view(-1)
        if bad.numel():
            off = int(bad[0].item())
            near = min(self._spans.items(), key=lambda kv: min(abs(off - kv[1][0]), abs(off - kv[1][0] - kv[1][1])))
            name, (start, nbytes, _, _) = near
            where = "%d bytes before its start" % (start - off) if off < start else "%d bytes past its end" % (off - start - nbytes + 1)
            raise AssertionError("%d guard bytes were overwritten; the first one lies %s of `%s` (%d bytes)" %
                                 (bad.numel(), where, name, nbytes))


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def call(name, *args):
    """One export of the C ABI on the current stream: tensors become device pointers, None a NULL pointer, LayerSpec-made
    descriptors are passed by reference; the stream argument is appended.  Raises on a non-zero return value."""
    from epipolar_transformers_amd import _lib

    conv = []
    for a in args:
        if a is None or isinstance(a, torch.Tensor):
            conv.append(ptr(a))
        elif isinstance(a, _lib.EtLayerDesc):
            conv.append(ctypes.byref(a))
        else:
            conv.append(a)
    conv.append(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(getattr(_lib.load(), name)(*conv), name)
