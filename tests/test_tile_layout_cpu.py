"""csrc/et_tile_layout.h is the one definition of the tile path's memory formats: the regions of the caller's workspace (and
the deterministic backward's tail) and the dynamic LDS of the three tile kernel families.  The host's size functions and the
kernels' pointers both come from it, so what can still go wrong is the layout itself.  A host program compiled against the
header prints every layout the launchers can select, and the tests check, with the region sizes restated here from the
documented format: the regions come in the documented order and each has room for its contents, the alignments hold, and the
totals are the ones recorded below -- the values of the formulas the header replaced (workspace: what the exported size
functions returned; LDS: fwd_tile_lds_bytes, bwd_tile_lds_bytes, tile_ws_lds_bytes), so no byte of the formats moved."""
import os
import subprocess
import tempfile

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "epipolar_transformers_amd", "csrc")

SHAPES = ((1, 2, 2), (3, 10, 10), (2, 16, 16), (3, 64, 64), (3, 96, 96), (3, 128, 128))       # (N, H, W)
# (N, H, W) -> et_epipolar_forward_workspace_bytes, _stats_offset, et_epipolar_backward_tiled_det_workspace_bytes
WORKSPACE = {
    (1, 2, 2): (1272, 388, 10248),
    (3, 10, 10): (13344, 1840, 629584),
    (2, 16, 16): (19376, 2368, 1069264),
    (3, 64, 64): (452160, 50944, 25619824),
    (3, 96, 96): (1016640, 114304, 57641584),
    (3, 128, 128): (1806912, 203008, 102472048),
}
# (rows, words of the source-pixel bitmap, samples per lane) -> bytes.  The bitmap words are those of the smallest and the
# largest map that takes the instance: 256 rows up to 64 x 64 (16 x 16: 8, 64 x 64: 128), 384 beyond (96 x 96: 288,
# 128 x 128: 512), 512 with K > 96 above 96 x 96; 512 rows are instantiated for two and four samples per lane only.
FWD_LDS = {
    (256, 8, 1): 52096, (256, 8, 2): 35712, (256, 8, 4): 35712, (256, 128, 1): 53056, (256, 128, 2): 36672, (256, 128, 4): 36672,
    (384, 288, 1): 70720, (384, 288, 2): 54336, (384, 288, 4): 54336, (384, 512, 1): 72512, (384, 512, 2): 56128, (384, 512, 4): 56128,
    (512, 512, 2): 73024, (512, 512, 4): 73024,
}
# ... and the merged form: 192 rows up to 64 x 64, 288 beyond and as the second launch of a 64 x 64 call
BWD_LDS = {
    (256, 8, 1): 51632, (256, 8, 2): 35248, (256, 8, 4): 35248, (256, 128, 1): 52592, (256, 128, 2): 36208, (256, 128, 4): 36208,
    (384, 288, 1): 70384, (384, 288, 2): 54000, (384, 288, 4): 54000, (384, 512, 1): 72176, (384, 512, 2): 55792, (384, 512, 4): 55792,
    (512, 512, 2): 72688, (512, 512, 4): 72688,
    (192, 8, 1): 51120, (192, 128, 1): 52080, (288, 128, 1): 77040, (288, 288, 1): 78320, (288, 512, 1): 80112,
}
# (rows, H, W, band table) -> bytes: the 256-row instance, the 288-row band instance, and the latter at 128 x 128 in two passes
WS_LDS = {
    (256, 16, 16, 0): 140032, (256, 64, 64, 0): 157312,
    (288, 16, 16, 1): 156896, (288, 96, 96, 1): 156896, (288, 128, 128, 1): 156896,
}
LDS_PER_CU = 160 * 1024

SRC = r"""
#include <cstdio>
#include "et_tile_layout.h"

#define F(l, f) std::printf(" " #f "=%%zu", (size_t)(l).f)

int main()
{
    static const int shapes[][3] = { %(shapes)s };
    for (const auto &s : shapes) {
        const size_t pairs = s[0], hw = (size_t)s[1] * s[2], tiles = pairs * ((hw + kTilePix - 1) / kTilePix);
        const TileWorkspaceLayout l = tile_workspace_layout(tiles, pairs, hw);
        const DetWorkspaceLayout d = det_workspace_layout(l.end, pairs, hw);
        std::printf("workspace %%d,%%d,%%d", s[0], s[1], s[2]);
        F(l, perm); F(l, ovf_list); F(l, stats); F(l, scales); F(l, segs); F(l, band); F(l, segs_pix); F(l, end); F(l, bytes);
        F(d, acc); F(d, quanta); F(d, partial); std::printf(" det_end=%%zu", d.end); F(d, extra_bytes);
        std::printf("\n");
    }
    // `segs` for every count of pairs (the scales in front of it are 16 bytes per pair; tiles decide the rest)
    int aligned = 1;
    for (size_t pairs = 1; pairs <= 64; ++pairs)
        for (size_t tiles_per_pair = 1; tiles_per_pair <= 9; ++tiles_per_pair)
            if (tile_workspace_layout(pairs * tiles_per_pair, pairs, 32 * tiles_per_pair).segs %% 16) aligned = 0;
    std::printf("segs_aligned x aligned=%%d\n", aligned);
    std::printf("header x words=%%d count=%%d err=%%d xcd_ctr=%%d xcds=%%d quads=%%d early=%%d overcap=%%d det_hard=%%d clear_end=%%d\n",
                kTileHdrWords, kTileHdrCount, kTileHdrErr, kTileHdrXcdCtr, kTileXcds, kTileHdrBwdQuads, kTileHdrBwdEarly,
                kTileHdrBwdOverCap, kTileHdrDetHard, kTileHdrClearEnd);
    static const int fwd[][3] = { %(fwd)s };
    for (const auto &k : fwd) {
        const FwdTileLds l = fwd_tile_lds(k[0], k[1], k[2]);
        std::printf("fwd %%d,%%d,%%d", k[0], k[1], k[2]);
        F(l, arr); F(l, rows); F(l, pix); F(l, U); F(l, ainv); F(l, seg); F(l, bitmap); F(l, prefix); F(l, nxy); F(l, end);
        std::printf("\n");
    }
    static const int bwd[][3] = { %(bwd)s };
    for (const auto &k : bwd) {
        const BwdTileLds l = bwd_tile_lds(k[0], k[1], k[2]);
        std::printf("bwd %%d,%%d,%%d", k[0], k[1], k[2]);
        F(l, arr); F(l, rows); F(l, pix); F(l, U); F(l, group_rows); F(l, drawn); F(l, red2); F(l, red1); F(l, ainv); F(l, seg);
        F(l, bitmap); F(l, prefix); F(l, nxy); F(l, end);
        std::printf("\n");
    }
    static const int ws[][4] = { %(ws)s };
    for (const auto &k : ws) {
        const TileWsLds l = tile_ws_lds(k[0], k[1], k[2], k[3] != 0);
        std::printf("ws %%d,%%d,%%d,%%d", k[0], k[1], k[2], k[3]);
        F(l, arr); F(l, rows); F(l, pix); F(l, seg); F(l, U); F(l, tq); F(l, ainv); F(l, band); F(l, dead); F(l, alpha); F(l, rinv);
        F(l, col); F(l, slot); F(l, astage); F(l, stash); F(l, end); F(l, bytes);
        std::printf(" slot_entries=%%d stage_bytes=%%d stash_bytes=%%d\n", tile_ws_slot_table_entries(k[1], k[2], k[3] != 0),
                    kWsAStageBytes, kWsStashBytes);
    }
    return 0;
}
"""


def _rows(keys):
    return ", ".join("{%s}" % ", ".join(str(int(v)) for v in k) for k in keys)


@pytest.fixture(scope="module")
def layouts():
    """(kind, key) -> the printed fields, in the order the header's struct declares them"""
    src_text = SRC % {"shapes": _rows(SHAPES), "fwd": _rows(FWD_LDS), "bwd": _rows(BWD_LDS), "ws": _rows(WS_LDS)}
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
        with open(src, "w") as fh:
            fh.write(src_text)
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, src])
        out = subprocess.check_output([exe], text=True)
    res = {}
    for line in out.splitlines():
        kind, key, *fields = line.split()
        key = tuple(int(v) for v in key.split(",")) if key != "x" else None
        res[(kind, key)] = {k: int(v) for k, v in (f.split("=") for f in fields)}
    return res


def _check_regions(layout, sizes, end):
    """`sizes`: region -> bytes of its contents, in the documented order; every region starts where the one before it has ended
    (or later: alignment), and the last one ends inside `end`."""
    names = list(sizes)
    for a, b in zip(names, names[1:] + [end]):
        assert layout[a] + sizes[a] <= layout[b], (a, b, layout)
    for a in names:
        assert layout[a] % 4 == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_workspace_regions_and_recorded_sizes(layouts, shape):
    n, h, w = shape
    hw = h * w
    tiles = n * ((hw + 31) // 32)
    l = layouts[("workspace", shape)]
    assert l["perm"] == 64 * 4                                      # behind the 64 header words
    _check_regions(l, {"perm": 4 * 32 * tiles, "ovf_list": 4 * tiles, "stats": 4 * tiles, "scales": 16 * n,
                       "segs": max(16 * 32 * tiles, 8 * n * hw), "band": 16 * tiles, "segs_pix": 16 * n * hw}, "end")
    # (segs: a pair's region -- 32 float4 per tile -- first holds the pair's sort keys, 8 bytes per pixel)
    assert 16 * 32 * (tiles // n) >= 8 * hw
    assert l["segs"] % 16 == 0 and l["band"] % 16 == 0 and l["segs_pix"] % 16 == 0
    total, stats, det_total = WORKSPACE[shape]
    assert l["bytes"] == total and l["end"] + 256 == total          # 256: the caller's base is rounded up
    assert l["stats"] == stats
    # the deterministic tail: from the next 256-byte boundary behind the forward's layout, inside the recorded total
    assert l["acc"] % 256 == 0 and l["end"] <= l["acc"] < l["end"] + 256
    _check_regions(l, {"acc": 8 * n * hw * 256, "quanta": 16 * n, "partial": 16 * 32 * n}, "det_end")
    assert l["bytes"] + l["extra_bytes"] == det_total
    assert l["det_end"] + 256 <= det_total


def test_segments_are_16_byte_aligned_for_every_pair_count(layouts):
    assert layouts[("segs_aligned", None)]["aligned"] == 1


def test_header_words(layouts):
    """Words 0 and 1 are the ABI (ops.py reads them); the counters of one call lie in the range the ordering clears, clear of the
    sticky error word."""
    hd = layouts[("header", None)]
    assert (hd["words"], hd["count"], hd["err"]) == (64, 0, 1)
    assert (hd["xcd_ctr"], hd["xcds"]) == (2, 8)
    assert (hd["quads"], hd["early"], hd["overcap"], hd["det_hard"]) == (2, 3, 4, 2)
    used = {hd["count"], hd["quads"], hd["early"], hd["overcap"], hd["det_hard"]} | set(range(hd["xcd_ctr"], hd["xcd_ctr"] + hd["xcds"]))
    assert hd["err"] not in used and max(used) < hd["clear_end"] == 10 <= hd["words"]


@pytest.mark.parametrize("key", sorted(FWD_LDS))
def test_forward_tile_lds(layouts, key):
    rows, hw_words, kpl = key
    l = layouts[("fwd", key)]
    array = max(4 * 32 * (rows + 4), 2 * 32 * 528)                  # the D/B array, or the fp16 stage of the split first GEMM
    _check_regions(l, {"arr": array, "rows": 4 * rows, "pix": 4 * 32, "U": 4, "ainv": 4 * 32, "seg": 16 * 32,
                       "bitmap": 4 * hw_words, "prefix": 4 * hw_words, "nxy": 8 * 32 * 64 if kpl == 1 else 0}, "end")
    assert l["arr"] == 0 and l["arr"] % 16 == 0 and l["nxy"] % 8 == 0
    assert l["end"] == FWD_LDS[key] <= LDS_PER_CU


@pytest.mark.parametrize("key", sorted(BWD_LDS))
def test_backward_tile_lds(layouts, key):
    rows, hw_words, kpl = key
    merged = rows in (192, 288)
    l = layouts[("bwd", key)]
    array = max(4 * 32 * (rows + 1) * (2 if merged else 1), 4 * 32 * 260)      # the array(s), or the staged A tile
    if merged or rows >= 384:
        assert array >= 2 * 32 * 528                                # ... and the fp16 stage where the D-type GEMMs are split
    table = kpl == 1 and not merged
    _check_regions(l, {"arr": array, "rows": 4 * rows, "pix": 4 * 32, "U": 4, "group_rows": 4, "drawn": 4, "red2": 4 * 8,
                       "red1": 4 * 4, "ainv": 4 * 32, "seg": 16 * 32, "bitmap": 4 * hw_words, "prefix": 4 * hw_words,
                       "nxy": 8 * 32 * 64 if table else 0}, "end")
    assert l["arr"] == 0 and l["nxy"] % 8 == 0
    assert l["end"] == BWD_LDS[key] <= LDS_PER_CU


@pytest.mark.parametrize("key", sorted(WS_LDS))
def test_persistent_forward_lds(layouts, key):
    rows, h, w, band = key
    l = layouts[("ws", key)]
    entries = 136 * 18 if band else (h + 4) * (w + 4)               # at least the padded map; the header rounds the row up
    assert l["slot_entries"] >= entries and l["slot_entries"] % 2 == 0
    assert l["stage_bytes"] == 2 * 32 * 512                         # fp16 hi and lo of 32 rows (tests/test_lds_layout_cpu.py)
    _check_regions(l, {"arr": 2 * 4 * 32 * (rows + 4), "rows": 3 * 4 * rows, "pix": 3 * 4 * 32, "seg": 3 * 16 * 32, "U": 4 * 8,
                       "tq": 4 * 8, "ainv": 2 * 4 * 32, "band": 3 * 16, "dead": 4 * 4, "alpha": 4 * 32, "rinv": 4 * 32,
                       "col": 4 * (136 if band else 72), "slot": 2 * 2 * l["slot_entries"], "astage": 2 * l["stage_bytes"]}, "end")
    assert l["arr"] == 0 and l["seg"] % 16 == 0 and l["band"] % 16 == 0
    assert l["astage"] % 256 == 0                                   # G1 steps through a row's chunks by XOR on the whole offset
    # two passes: the stash of the first half's accumulators is the second stage
    assert l["stash"] == l["astage"] + l["stage_bytes"] and l["stash"] + l["stash_bytes"] <= l["end"]
    assert l["end"] <= l["bytes"] == WS_LDS[key] <= LDS_PER_CU
