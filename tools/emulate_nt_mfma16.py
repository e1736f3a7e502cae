#!/usr/bin/env python
"""CPU emulation of the K loop of the bf16 role-split NT kernels (csrc/gemm.hip, gemm_nt_stagger_kernel with the
16x16x32 MFMA shape): the LDS-DMA chunk placement, the fragment addresses of every L segment, the four-MFMA decomposition of
a 32x32 block and the v_permlane16_swap shuffle into the 32x32 accumulator layout -- with the index formulas the kernel
uses, transcribed.  For TM = 2, 3, 4 and both orientations (TR: MFMA operands swapped, lane = token) it checks

 (a) layout:    after the shuffle, register R of lane l of acc[i][j] holds col = l & 31, row = acc_row(R, l) of the wave's
                32x32 block (i, j) -- for every (register, lane), on operands whose every product element is unique, and on
                random integer operands over a whole 64-wide K-tile;
 (b) banks:     every ds_read_b128 of a K-tile is conflict-free under the MI355X lane groups of that instruction, for every
                16-row group of the A and B tiles;
 (c) placement: every (row, k-chunk) of a tile is read from where the DMA wrote it, and every chunk of the tile is read.

No GPU needed; run after touching the kernel's address math.

Layout models (pa_mma.h): 32x32 accumulator: col = lane & 31, row = (R & 3) + 8 (R >> 2) + 4 (lane >> 5);
v_mfma_f32_16x16x32_bf16: lane l supplies A[row l & 15][k = 8 (l >> 4) .. +8] and B[k = 8 (l >> 4) .. +8][col l & 15], the
result sits at col = l & 15, row = 4 (l >> 4) + reg; v_permlane16_swap X, Y exchanges the odd 16-lane rows of X with the
even 16-lane rows of Y.
"""
import numpy as np

KB = 128                                 # bytes of K per ring stage: 64 bf16
WN = 4                                   # waves per group; 2 groups
# ds_read_b128: four 16-lane groups, one LDS cycle each when conflict-free; bank of byte a: (a / 4) % 64
B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
               [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]


# ---- the kernel's address functions ----------------------------------------------------------------------------------
def swz_nt128(row):
    return (row >> 1) & 7


def perm16(x):
    return (x & 3) | ((x & 4) << 1) | ((x & 8) >> 1)


def acc_row(r, lane):
    return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)


def dma_piece(wave, i, per, lane):
    """wave-instruction i (of `per` per wave and stage) of a tile's LDS-DMA: 1 KiB of contiguous LDS.
    Returns (LDS byte address within the tile, tile row, logical 16-byte chunk fetched from that row)."""
    q = (wave * per + i) * 64 + lane
    row = q >> 3
    c = (q & 7) ^ swz_nt128(row)
    return (wave * per + i) * 1024 + lane * 16, row, c


def frag_off(tile_row0, r16, s, lane):
    """offA16[s] / offB16[s]: byte address of a lane's fragment of 16-row group 0 of its wave tile in substep s"""
    return (tile_row0 + r16) * 128 + (((4 * s + (lane >> 4)) ^ swz_nt128(r16)) << 4)


def lane_rows(TR, lane):
    """(rA16, rB16): row within a 16-row group that the lane reads of the A (token) and B (weight) tiles"""
    x = lane & 15
    return (x, perm16(x)) if TR else (perm16(x), x)


# ---- instruction models ------------------------------------------------------------------------------------------------
def mfma16(row_frag, col_frag):
    """row_frag, col_frag: (64 lanes, 8) -> D (64 lanes, 4 regs)"""
    R, C = np.zeros((16, 32)), np.zeros((16, 32))
    for l in range(64):
        R[l & 15, 8 * (l >> 4):8 * (l >> 4) + 8] = row_frag[l]
        C[l & 15, 8 * (l >> 4):8 * (l >> 4) + 8] = col_frag[l]
    D = R @ C.T
    out = np.zeros((64, 4))
    for l in range(64):
        for r in range(4):
            out[l, r] = D[4 * (l >> 4) + r, l & 15]
    return out


def permlane16_swap(x, y):
    x, y = x.copy(), y.copy()
    for base in (0, 32):
        lo, hi = slice(base, base + 16), slice(base + 16, base + 32)
        x[hi], y[lo] = y[lo].copy(), x[hi].copy()
    return x, y


def acc32_from_16(acc, p, d0, d1):
    for r in range(4):
        x, y = permlane16_swap(d0[:, r], d1[:, r])
        acc[:, 8 * p + r], acc[:, 8 * p + 4 + r] = x, y


def bank_conflict_degree(addrs):
    worst = 1
    for grp in B128_GROUPS:
        per_bank = {}
        for l in grp:
            for dw in range(addrs[l] // 4, addrs[l] // 4 + 4):
                per_bank.setdefault(dw % 64, set()).add(dw)
        worst = max(worst, max(len(v) for v in per_bank.values()))
    return worst


# ---- one workgroup, one K-tile -----------------------------------------------------------------------------------------
def fill_tile(M, rows, per):
    """LDS image of a [rows][64] operand tile as the DMA leaves it: values (flat, one entry per bf16) and (row, chunk) tags per
    16-byte slot.  Every instruction writes 8 rows x 128 contiguous bytes and fetches 16 bytes per lane"""
    vals = np.full(rows * 64, np.nan)
    tags = [None] * (rows * 8)
    for wave in range(8):
        for i in range(per):
            seen_rows = set()
            for lane in range(64):
                a, row, c = dma_piece(wave, i, per, lane)
                assert tags[a // 16] is None
                tags[a // 16] = (row, c)
                vals[a // 2:a // 2 + 8] = M[row, 8 * c:8 * c + 8]
                seen_rows.add(row)
            assert len(seen_rows) == 8 and max(seen_rows) - min(seen_rows) == 7       # 8 whole rows per instruction
    assert all(t is not None for t in tags) and len(set(tags)) == rows * 8
    return vals, tags


def run_workgroup(TM, TR, A, B, phases=4):
    """A [64 TM][64], B [256][64] (one K-tile).  Returns (C as the accumulators say, worst bank conflict degree, set of A slots read,
    set of B slots read); asserts (c) on the way"""
    TBM = 64 * TM
    ldsA, tagA = fill_tile(A, TBM, TM)
    ldsB, tagB = fill_tile(B, 256, 4)
    C = np.full((TBM, 256), np.nan)
    worst = 1
    readA, readB = set(), set()
    pps = phases // 2
    ng = 2 * TM // pps
    for wave in range(8):
        wr, wc = wave // WN, wave % WN
        d16 = [[np.zeros((64, 4)) for _ in range(4)] for _ in range(2 * TM)]
        fb16 = None
        for ph in range(phases):
            s, g0 = ph // pps, (ph % pps) * ng

            def read(lds, tags, seen, row0, which, g):
                addrs, frag = [], np.zeros((64, 8))
                for lane in range(64):
                    r16 = lane_rows(TR, lane)[which]
                    a = frag_off(row0, r16, s, lane) + g * 16 * 128
                    assert tags[a // 16] == (row0 + 16 * g + r16, 4 * s + (lane >> 4)), "fragment read off its DMA slot"
                    seen.add(a // 16)
                    addrs.append(a)
                    frag[lane] = lds[a // 2:a // 2 + 8]
                return frag, bank_conflict_degree(addrs)

            fa16 = []
            for x in range(ng):
                f, w = read(ldsA, tagA, readA, wr * TM * 32, 0, g0 + x)
                fa16.append(f)
                worst = max(worst, w)
            if ph % pps == 0:
                fb16 = []
                for b in range(4):
                    f, w = read(ldsB, tagB, readB, wc * 64, 1, b)
                    fb16.append(f)
                    worst = max(worst, w)
            for x in range(ng):
                for b in range(4):
                    d16[g0 + x][b] += mfma16(fb16[b], fa16[x]) if TR else mfma16(fa16[x], fb16[b])
        for i in range(TM):
            for j in range(2):
                acc = np.zeros((64, 16))
                for p in range(2):
                    if TR:
                        acc32_from_16(acc, p, d16[2 * i][2 * j + p], d16[2 * i + 1][2 * j + p])
                    else:
                        acc32_from_16(acc, p, d16[2 * i + p][2 * j], d16[2 * i + p][2 * j + 1])
                # what every epilogue assumes of acc[i][j]
                for lane in range(64):
                    for R in range(16):
                        if TR:
                            m, n = lane & 31, acc_row(R, lane)
                        else:
                            m, n = acc_row(R, lane), lane & 31
                        row, col = wr * TM * 32 + i * 32 + m, wc * 64 + j * 32 + n
                        assert np.isnan(C[row, col])
                        C[row, col] = acc[lane, R]
    return C, worst, readA, readB


def check(TM, TR, phases=4):
    TBM = 64 * TM
    rng = np.random.default_rng(TM * 2 + TR)
    # (a1) unique products: C[m][n] = (m + 1) + 1000 (n + 1), carried by k = 0 and k = 63 (first and last chunk)
    A, B = np.zeros((TBM, 64)), np.zeros((256, 64))
    A[:, 0], B[:, 0] = np.arange(TBM) + 1, 1
    A[:, 63], B[:, 63] = 1, 1000 * (np.arange(256) + 1)
    C, worst, ra, rb = run_workgroup(TM, TR, A, B, phases)
    np.testing.assert_array_equal(C, A @ B.T)
    assert len(np.unique(C)) == C.size
    # (a2) every k: integers, exact
    A, B = rng.integers(-8, 9, (TBM, 64)).astype(np.float64), rng.integers(-8, 9, (256, 64)).astype(np.float64)
    C, worst2, ra, rb = run_workgroup(TM, TR, A, B, phases)
    np.testing.assert_array_equal(C, A @ B.T)
    # (b)
    assert max(worst, worst2) == 1, f"TM={TM} TR={TR}: {max(worst, worst2)}-way bank conflict in a fragment read"
    # (c) coverage: every 16-byte slot of both tiles is read by some wave
    assert len(ra) == TBM * 8 and len(rb) == 256 * 8
    return max(worst, worst2)


def main():
    for TM in (2, 3, 4):
        for TR in (False, True):
            for phases in (2, 4):
                check(TM, TR, phases)
            print(f"TM={TM} TR={int(TR)}: layout, bank conflicts (1-way), DMA placement OK")


if __name__ == "__main__":
    main()
