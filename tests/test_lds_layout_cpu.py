"""csrc/et_lds_layout.h places the fp16 operands of the persistent forward kernel in LDS and defines G1's lane trade.  Its
claims -- every ds_read_b128 of an MFMA fragment costs 4 LDS-array cycles, the writers stay within their bounds, the trade
hands every lane the chunk it needs -- are checked here on the CPU against the gfx950 bank model: a C program compiled against
the header evaluates the lane-group table below for the kernel's address expressions.  The PREVIOUS expressions (528-byte rows,
`& 7` swizzle, holder 4 n + kg) are evaluated with the same model and must come out at 8 cycles: what a reader will doubt is
the model, and that is the figure the hardware counters were explained with.

The model:  ds_read_b128   four groups of sixteen lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, the same + 32;
                           bank (a / 4) mod 64, four banks per lane
            ds_write_b64   four groups of sixteen contiguous lanes; bank (a / 4) mod 32, two banks per lane
            ds_write_b32 / ds_bpermute   two groups of 32 contiguous lanes; bank (a / 4) mod 32
            a group takes as many cycles as its busiest bank has distinct addresses; identical addresses broadcast."""
import os
import subprocess
import tempfile

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "epipolar_transformers_amd", "csrc")

SRC = r"""
#include <stdio.h>
#include <string.h>
#include "et_lds_layout.h"

/* cycles of one wave instruction: `ngroups` lane groups (group_of[lane]), `width` bytes per lane, `banks` banks of 4 bytes */
static int cycles(const int *addr, const int *group_of, int ngroups, int width, int banks)
{
    int total = 0;
    for (int g = 0; g < ngroups; ++g) {
        int worst = 0;
        for (int b = 0; b < banks; ++b) {
            int seen[64], ns = 0;
            for (int l = 0; l < 64; ++l) {
                if (group_of[l] != g) continue;
                for (int w = 0; w < width / 4; ++w) {
                    const int dw = addr[l] / 4 + w;
                    if (dw % banks != b) continue;
                    int k = 0;
                    while (k < ns && seen[k] != dw) ++k;
                    if (k == ns) seen[ns++] = dw;
                }
            }
            if (ns > worst) worst = ns;
        }
        total += worst;
    }
    return total;
}
static int grp_read128[64], grp16[64], grp32[64];
static void groups(void)
{
    for (int l = 0; l < 64; ++l) {
        const int q = l & 31;
        const int first = q < 4 || (q >= 12 && q < 16) || (q >= 20 && q < 28);
        grp_read128[l] = 2 * (l >> 5) + (first ? 0 : 1);
        grp16[l] = l >> 4;
        grp32[l] = l >> 5;
    }
}
static int read_b128(const int *a) { return cycles(a, grp_read128, 4, 16, 64); }
static int write_b64(const int *a) { return cycles(a, grp16, 4, 8, 32); }
static int b32(const int *a) { return cycles(a, grp32, 2, 4, 32); }

/* the expressions the kernel used before this header */
static int old_astage_off(int n, int ks, int kg) { return n * 528 + ks * 64 + kg * 16; }
static int old_g3_off(int m, int c) { return m * 512 + ((c ^ (m & 7)) << 4); }
static int old_source_lane(int n, int kg) { return 4 * n + kg; }

#define UPD(lo, hi, v) do { const int v_ = (v); if (v_ < lo) lo = v_; if (v_ > hi) hi = v_; } while (0)

int main(void)
{
    groups();
    int a[64];
    /* (a) every row's 32 chunks exactly once, inside the row; the reader's XOR form */
    int bij = 1, inside = 1, xor_form = 1;
    for (int n = 0; n < 32; ++n) {
        unsigned seen = 0;
        for (int ks = 0; ks < 8; ++ks)
            for (int kg = 0; kg < 4; ++kg) {
                const int s = et_astage_slot(n, ks, kg), off = et_astage_off(n, ks, kg);
                if (s < 0 || s > 31 || off < n * ET_ASTAGE_ROW_BYTES || off + 16 > (n + 1) * ET_ASTAGE_ROW_BYTES || off % 16) inside = 0;
                else seen |= 1u << s;
                if (off != (et_astage_off(n, 0, kg) ^ et_astage_kstep_xor(ks))) xor_form = 0;
            }
        if (seen != 0xffffffffu) bij = 0;
    }
    printf("astage_bijection %d\nastage_inside %d\nastage_xor_form %d\nastage_bytes %d\n", bij, inside, xor_form, 32 * ET_ASTAGE_ROW_BYTES);
    /* (b) G1's A fragments: MFMA lane (n, kg) = (lane & 15, lane >> 4), pixel half g, k-step ks */
    int lo = 99, hi = 0, olo = 99, ohi = 0;
    for (int g = 0; g < 2; ++g)
        for (int ks = 0; ks < 8; ++ks) {
            for (int l = 0; l < 64; ++l) a[l] = et_astage_off((l & 15) + 16 * g, ks, l >> 4);
            UPD(lo, hi, read_b128(a));
            for (int l = 0; l < 64; ++l) a[l] = old_astage_off((l & 15) + 16 * g, ks, l >> 4);
            UPD(olo, ohi, read_b128(a));
        }
    printf("g1_read_min %d\ng1_read_max %d\nold_g1_read_min %d\nold_g1_read_max %d\n", lo, hi, olo, ohi);
    /* (c) the A stage's writer: one row per instruction, lane = 4 channels = 8 bytes: ks = lane >> 3, e = (lane >> 2) & 1, kg = lane & 3 */
    lo = 99, hi = 0, olo = 99, ohi = 0;
    for (int n = 0; n < 32; ++n) {
        for (int l = 0; l < 64; ++l) a[l] = et_astage_off(n, l >> 3, l & 3) + 8 * ((l >> 2) & 1);
        UPD(lo, hi, write_b64(a));
        for (int l = 0; l < 64; ++l) a[l] = old_astage_off(n, l >> 3, l & 3) + 8 * ((l >> 2) & 1);
        UPD(olo, ohi, write_b64(a));
    }
    printf("astage_write_max %d\nold_astage_write_max %d\n", hi, ohi);
    /* G3's staged out tile: rows' chunks exactly once; fragment read of lane (li, lh) = chunk 2 ks + lh of row li */
    bij = 1;
    for (int m = 0; m < 32; ++m) {
        unsigned seen = 0;
        for (int c = 0; c < 32; ++c) {
            const int off = et_g3_stage_off(m, c) - m * 512;
            if (off < 0 || off >= 512 || off % 16) bij = 0;
            else seen |= 1u << (off / 16);
        }
        if (seen != 0xffffffffu) bij = 0;
    }
    lo = 99, hi = 0, olo = 99, ohi = 0;
    for (int ks = 0; ks < 16; ++ks) {
        for (int l = 0; l < 64; ++l) a[l] = et_g3_stage_off(l & 31, 2 * ks + (l >> 5));
        UPD(lo, hi, read_b128(a));
        for (int l = 0; l < 64; ++l) a[l] = old_g3_off(l & 31, 2 * ks + (l >> 5));
        UPD(olo, ohi, read_b128(a));
    }
    printf("g3_bijection %d\ng3_read_min %d\ng3_read_max %d\nold_g3_read_min %d\nold_g3_read_max %d\n", bij, lo, hi, olo, ohi);
    /* ... and its writer (4-byte stores: accumulator register r of matrix wave w, lane (cq, s, lh) -> row m, channel pair cb) */
    int wmax = 0, owmax = 0;
    for (int w = 0; w < 4; ++w)
        for (int r = 0; r < 16; ++r) {
            for (int l = 0; l < 64; ++l) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), cb = 64 * w + 4 * (l & 15) + 2 * ((l >> 4) & 1);
                a[l] = et_g3_stage_off(m, cb >> 3) + (cb & 7) * 2;
            }
            if (b32(a) > wmax) wmax = b32(a);
            for (int l = 0; l < 64; ++l) {
                const int m = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), cb = 64 * w + 4 * (l & 15) + 2 * ((l >> 4) & 1);
                a[l] = old_g3_off(m, cb >> 3) + (cb & 7) * 2;
            }
            if (b32(a) > owmax) owmax = b32(a);
        }
    printf("g3_write_max %d\nold_g3_write_max %d\n", wmax, owmax);
    /* (d), (e) the lane trade */
    int perm = 1, chunk_ok = 1, distinct = 1, old_distinct = 1;
    unsigned long long seen64 = 0;
    for (int half = 0; half < 2; ++half) {
        unsigned m32 = 0, om32 = 0;
        for (int q = 0; q < 32; ++q) {
            const int l = 32 * half + q, n = l & 15, kg = l >> 4, s = et_g1_source_lane(n, kg);
            if (s < 0 || s > 63) { perm = 0; continue; }
            seen64 |= 1ull << s;
            m32 |= 1u << (s & 31);
            om32 |= 1u << (old_source_lane(n, kg) & 31);
            if ((s >> 2) != n || et_g1_loaded_chunk(s) != kg) chunk_ok = 0;      /* holder s loaded chunk kg of row n */
        }
        if (m32 != 0xffffffffu) distinct = 0;
        if (om32 != 0xffffffffu) old_distinct = 0;
    }
    if (seen64 != ~0ull) perm = 0;
    for (int l = 0; l < 64; ++l) a[l] = 4 * et_g1_source_lane(l & 15, l >> 4);
    const int bp = b32(a);
    for (int l = 0; l < 64; ++l) a[l] = 4 * old_source_lane(l & 15, l >> 4);
    printf("trade_permutation %d\ntrade_chunk %d\ntrade_distinct %d\nold_trade_distinct %d\ntrade_cycles %d\nold_trade_cycles %d\n",
           perm, chunk_ok, distinct, old_distinct, bp, b32(a));
    int quad = 1;       /* a quad still loads the four chunks of one 64-byte segment */
    for (int q = 0; q < 16; ++q) {
        int m = 0;
        for (int j = 0; j < 4; ++j) m |= 1 << et_g1_loaded_chunk(4 * q + j);
        if (m != 15) quad = 0;
    }
    printf("trade_quads %d\n", quad);
    return 0;
}
"""


@pytest.fixture(scope="module")
def model():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(src, "w") as fh:
            fh.write(SRC)
        subprocess.check_call(["gcc", "-O2", "-std=c99","-I" + CSRC, "-o", exe, src])
        out = subprocess.check_output([exe], text=True)
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def test_a_stage_places_every_chunk_once_inside_its_row(model):
    assert model["astage_bijection"] == 1 and model["astage_inside"] == 1
    assert model["astage_xor_form"] == 1              # the reader's one-XOR-per-k-step form of the same offsets
    assert model["astage_bytes"] == 16384             # hi + lo, two stages: 65536; the two-pass stash is one stage pair, 32768


def test_g1_fragment_reads_cost_four_cycles(model):
    assert (model["g1_read_min"], model["g1_read_max"]) == (4, 4)


def test_a_stage_writer_stays_within_eight_cycles(model):
    assert model["astage_write_max"] <= 8


def test_g3_stage_is_a_bijection_and_reads_in_four_cycles(model):
    assert model["g3_bijection"] == 1
    assert (model["g3_read_min"], model["g3_read_max"]) == (4, 4)
    assert model["g3_write_max"] == model["old_g3_write_max"]      # within a 32-lane half the row is constant


def test_lane_trade_is_a_permutation_distinct_mod_32_per_half(model):
    assert model["trade_permutation"] == 1 and model["trade_distinct"] == 1 and model["trade_quads"] == 1
    assert model["trade_cycles"] == 2                 # one per 32-lane half under the 32-bank rule


def test_lane_trade_delivers_chunk_kg_of_row_n(model):
    assert model["trade_chunk"] == 1


def test_the_model_gives_eight_cycles_for_the_previous_layouts(model):
    assert (model["old_g1_read_min"], model["old_g1_read_max"]) == (8, 8)
    assert (model["old_g3_read_min"], model["old_g3_read_max"]) == (8, 8)
    assert model["old_astage_write_max"] == 4
    assert model["old_trade_distinct"] == 0 and model["old_trade_cycles"] == 4
