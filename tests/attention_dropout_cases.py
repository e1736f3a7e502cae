"""Cases, mask rule, references, bounds and checkers of the attention-dropout parity suite (pa_attention_fwd_dropout,
pa_attention_bwd_dropout, pa_attention_dropout_mask).  Built on tests/attention_cases.py: same operand families, same guarded buffers,
same calling conventions; a checker hands an `impl` a case plus (seed, site, t) and neither knows nor cares where the arithmetic ran.
Used by tests/test_gpu_attention_dropout.py (the HIP kernels through the C ABI) and tests/test_attention_dropout_cpu.py (the same
checkers against `TorchDropAttention`, plain torch with the specified arithmetic, and against its fault models).  Imports no HIP.

The mask rule (include/passt_amd.h), restated here in numpy from its text: t = round(256 p), 1 <= t <= 255, keep = 1 - t / 256;
element (site, s = b H + h, query q, key k) of the probabilities, q and k the indices inside the sequence:
    R    = philox4x32_10(counter = (k >> 2, q >> 2, s, site), key = (seed[0], seed[1]))
    byte = (R[q & 3] >> (8 (k & 3))) & 0xff
    kept <=> byte >= t
Philox4x32 with 10 rounds: multipliers D2511F53 / CD9E8D57, key increments 9E3779B9 / BB67AE85.

Specified arithmetic, D = kept / keep:  lse and the row sum l are those of the undropped softmax;  O = (P D) V, formed as
(sum_kept p v) / (l keep);  delta = rowsum(dO o) from the STORED o;  dP = D (dO V^T);  dS = P (dP - delta) (a dropped element has
dS = -P delta);  dV = (P D)^T dO;  dQ, dK from dS as without dropout.

Bounds: those of tests/attention_cases.py with P D wherever P multiplies V or dO and D dP for dP, and nothing else changed:
  o    (U + EPS) ((P D) |V|) + U |o|                       dV   (U + EPS) ((P D)^T |dO|) + U |dV|
  E_S = (U + EPS) |dS| + max(U, 2^-21) P . Delta            Delta = sum_d |dO o| with the dropped o
  dQ   scale (E_S |K|) + U |dQ|                             dK   scale (E_S^T |Q|) + U |dK|           (f32: U = 0)
Why they carry over.  The mask is a selection and 1 / keep one more f32 factor, so against the undropped kernels the arithmetic has
three more f32 roundings per element: of l keep (forward), of D dP = dP / keep, and of the sum D dP + (-delta) that the undropped
kernels take from the matrix pipe.  Each is 2^-24 relative to its own result: the first is 2^-10 EPS of o; the other two are at most
3 2^-24 (|D dP| + |delta|) <= 3 2^-24 (|dS| / P + 2 Delta) per element, i.e. times P at most 3 2^-10 EPS |dS| + 6 2^-24 P Delta,
both inside the terms above (EPS was derived with a factor 2 to spare, and 2^-21 = 8 2^-24).  P itself is formed from the same stored
lse by the same chain, so EPS (and eps_rows' score-chain term under the pre-scaled q) is unchanged.  For the select / pair families
outside the exact regime (below) the forward's f32 figure of attention_cases (2^-21 + eps_rows - EPS) joins U: the same pieces.
Underflow.  Without dropout a row's hot key carries its bound.  With it the hot key of a spiked row (the graded family's) can be
dropped, and the row is then made of probabilities of 1e-46 alone: below TINY = 2^-126, the smallest normal number of f32 and of bf16,
where an exponential, a product or a stored result is a denormal or zero in ANY implementation (attention_cases zeroes them in the
reference of its exact families: "no bound could see it").  So every bound outside the exact regime gets the format's own floor: a
probability is off by at most TINY absolutely, i.e. o by TINY sum_k D |v|, dV by TINY sum_q D |dO|, dS by TINY (|D dP| + Delta), and
every stored result by TINY once more.

Exactness.  The select, pair and uniform families keep the exactness claims of attention_cases.py when 1 / keep is a power of two
(asserted by exact_regime(): t = 128, 192, 224, ...; 1 - 64 / 256 = 3 / 4 is not, so t = 64 is judged by the bounds): then D is 0 or a
power of two, every product with it is exact, and the conditions of the families hold with |v|, |dO| doubled (asserted in
drop_conditions).  bf16: torch.equal against the f64 result rounded once; f32: exactly 0 where the reference has no term, EPS A +
floor elsewhere; uniform: o exact for N a power of two, else a neighbour of the f64 value.  Outside that regime every family is judged
by the bounds above.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

from tests import attention_cases as A
from tests.attention_cases import (BF16, EPS, F32, F64, HD, LN2, LOG2E, O_F32, PA_BF16, PA_F32, PA_OK, PRE, SCALE, TD, U, GuardedOut,  # noqa: F401
                                   equal, from_rows, lp, lse_of, mm, new_out, within)

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
SEED = (0x2545F491, 0x4F6CDD1D)       # the suite's seed; tests/test_attention_dropout_cpu.py asserts the kept-fraction condition on it
SEED2 = (0x2545F492, 0x4F6CDD1D)
TINY = 2.0 ** -126                    # smallest normal number of f32 and bf16
T_EXACT, T_GRADED = 128, 26           # keep = 1/2 (exact regime) and round(256 * 0.1)
N_FWD_BWD = (1, 2, 33, 64, 65, 129, 257, 513)
BH_DROP = ((1, 1), (2, 3))


# ---- the rule --------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """numpy uint64 arrays (values < 2^32), broadcast against each other -> the four result words"""
    c = [np.asarray(x, dtype=np.uint64) for x in (c0, c1, c2, c3)]
    k = [np.uint64(k0), np.uint64(k1)]
    lo32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & lo32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & lo32]
        k = [(k[0] + np.uint64(W0)) & lo32, (k[1] + np.uint64(W1)) & lo32]
    return c


def rule_bytes(seed, site, BH, nq, N, s0=0, q_of=None, k_of=None):
    """the byte of every element, uint8 numpy (BH, nq, N), for heads s0 .. s0 + BH - 1.  q_of / k_of: the query / key index the rule is
    evaluated at, as functions of the (q, k) grids -- the fault models' index mix-ups (identity by default)"""
    z = np.zeros((BH, nq, N), dtype=np.uint64)
    s = z + np.arange(s0, s0 + BH, dtype=np.uint64)[:, None, None]
    q0 = z + np.arange(nq, dtype=np.uint64)[None, :, None]
    k0 = z + np.arange(N, dtype=np.uint64)[None, None, :]
    q = q0 if q_of is None else q_of(q0, k0).astype(np.uint64)
    k = k0 if k_of is None else k_of(q0, k0).astype(np.uint64)
    R = np.stack(philox4x32_10(k >> np.uint64(2), q >> np.uint64(2), s, z + np.uint64(site), seed[0], seed[1]), 0)
    word = np.take_along_axis(R, (q & np.uint64(3)).astype(np.int64)[None], 0)[0]
    return ((word >> (np.uint64(8) * (k & np.uint64(3)))) & np.uint64(0xff)).astype(np.uint8)


@functools.lru_cache(maxsize=64)
def rule_mask(seed, site, BH, nq, N, t):
    """the keep mask, torch bool (BH, nq, N), from the restatement above"""
    return torch.from_numpy(rule_bytes(seed, site, BH, nq, N) >= t)


def keep_of(t):
    return 1.0 - t / 256.0


def exact_regime(t):
    """1 / keep is a power of two: every product with D is exact"""
    k = 256 - t
    return k & (k - 1) == 0


# ---- cases -----------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class DC:
    """an attention case of tests/attention_cases.py (fixed length) under dropout: threshold t, seed, site"""
    c: A.AC
    t: int
    seed: tuple = SEED
    site: int = 0

    @property
    def name(self):
        return f"{self.c.name},t{self.t},site{self.site}"

    @property
    def keep(self):
        return keep_of(self.t)


def mask_of(d, b):
    """[H][nq_b][N] keep mask of sequence b"""
    c = d.c
    return rule_mask(d.seed, d.site, c.B * c.H, c.nqk, c.N, d.t)[b * c.H:(b + 1) * c.H]


def fwd_bwd_cases(N, ts=(T_EXACT, T_GRADED)):
    """both types, with and without the pre-scaled q, every family, nq = N and nq = 2, two (B, H), t innermost (the f64 softmax
    is shared)"""
    j = N_FWD_BWD.index(N)
    out = []
    for dt in (PA_F32, PA_BF16):
        for pre in (0, PRE):
            for i, nq in enumerate((0, 2)):
                if nq and nq >= N:
                    continue
                B, H = BH_DROP[(j + i + pre + dt) % 2]
                for c in A._family_cases(dt, B, H, N, pre, j, nq=nq):
                    # (o + e of the oshift variant is a number of the type only where 1 / keep is a power of two)
                    out += [DC(c, t, site=(j + i) % 5) for t in ts if exact_regime(t) or not c.oshift]
    return out


# ---- f64 reference ---------------------------------------------------------------------------------------------------------
def drop_reference(d, masks=None):
    """per sequence: attention_cases' reference with the explicit mask (masks: per-sequence [H][nq][N] bool, default the rule's)"""
    c, out = d.c, []
    i, r = A.attn_inputs(c), A.reference(c)
    for b, rb in enumerate(r):
        m = (mask_of(d, b) if masks is None else masks[b])
        D = m.double() / d.keep
        P, v, k, q, d_o = rb["P"], rb["v"], rb["k"], rb["q"] / i["qfac"], rb["d_o"]
        fac = SCALE * i["qfac"]
        PD = P * D
        # as attention_cases forms o: the sum of the unnormalised terms first, ONE division behind it (exact sums stay exact)
        pu = torch.exp(rb["s"] - rb["s"].max(-1, keepdim=True).values)
        if c.fam in ("select", "pair"):
            pu = torch.where(pu < 2.0 ** -126, torch.zeros_like(pu), pu)
        o = ((pu * m.double()) @ v) / (pu.sum(-1, keepdim=True) * d.keep)
        o_in = o + i["info"][b]["e"].double() if c.oshift else o
        dP = D * rb["dP"]
        delta = (d_o * o_in).sum(-1)
        dS = P * (dP - delta[..., None])
        nq = c.nq_b(b)
        dq = torch.zeros_like(rb["dq"])
        dq[:, :nq] = SCALE * (dS @ k)
        dD = D * rb["dP"].abs()
        under = dict(o=TINY * (1 + (D @ v.abs())), dv=TINY * (1 + D.transpose(1, 2) @ d_o.abs()), dS=TINY * (dD + (d_o * o_in).abs().sum(-1)[..., None]))
        out.append(dict(under=under, PD=PD, o=o, o_in=o_in, dS=dS, dabs=(d_o * o_in).abs().sum(-1), dq=dq, dk=fac * (dS.transpose(1, 2) @ q),
                        dv=PD.transpose(1, 2) @ d_o, A_o=PD @ v.abs(), mask=m))
    return out


def drop_conditions(d, r, rd):
    """the families' own conditions (attention_cases.conditions) plus what the exact regime needs"""
    c = d.c
    A.conditions(c, A.attn_inputs(c), r)
    if not exact_regime(d.t):
        return
    inv = 1.0 / d.keep
    assert inv == 2.0 ** round(np.log2(inv)), "1 / keep is a power of two"
    for b, rb in enumerate(r):
        N = c.seq[b]
        if c.fam == "pair":
            # exact f32 accumulation: sums of at most N terms, each a multiple of 2^-4 below 2^8 / keep
            assert N * 2 ** 8 * inv * 2 ** 4 < 2 ** 24
        if c.fam in ("select", "uniform"):
            # integer sums times 1 / keep stay below 2^24
            assert float(rd[b]["dv"].abs().max()) < 2 ** 24 and float(rd[b]["A_o"].max()) * N < 2 ** 24


# ---- plain torch with the specified arithmetic ---------------------------------------------------------------------------------
class TorchDropAttention(A.TorchAttention):
    """pa_attention_fwd_dropout / _bwd_dropout in plain torch on the CPU.  The small methods are the places a dropout kernel goes wrong;
    the fault models of tests/test_attention_dropout_cpu.py override them one at a time."""
    name = "torch-dropout"

    # -- hooks
    def mask(self, d, b, phase):
        """[H][nq_b][N_b] keep mask the kernel applies in `phase` (fwd | bwd)"""
        return mask_of(d, b)

    def rkeep_bwd(self, d):
        return torch.tensor(1.0 / d.keep, dtype=F32)

    def ds(self, P, x, ndelta, m):
        """dS / scale from P, x = D dP and -delta"""
        return P * (x + ndelta)

    # -- arithmetic
    def fwd_drop(self, d):
        c = d.c
        qkv = A.attn_inputs(c)["qkv"]
        td = TD[c.dt]
        o = new_out(c.o_rows, c.D, A.PAD_O, td, self.dev)
        lse = GuardedOut(c.n_lse, F32, self.dev)
        self.o_f32 = []
        keep = torch.tensor(d.keep, dtype=F32)
        for b in range(c.B):
            t = self.seq3(c, qkv, b)
            q = self.queries(c, b, t, "fwd")
            k, v = self.keys(c, b, t[1], t[2], "fwd")
            s2 = self.scores2(c, q, k)
            m = s2.max(-1, keepdim=True).values
            p = torch.exp2(s2 - m)
            l = p.double().sum(-1, keepdim=True).float()                      # of the undropped p
            lb = ((m + torch.log2(l)) * torch.tensor(LN2, dtype=F32))[..., 0]
            pd = torch.where(self.mask(d, b, "fwd"), p, torch.zeros_like(p))   # selected, not multiplied
            ob = mm(self.p_lp(pd, td), v) / (l * keep)
            nq = c.nq_b(b)
            self.o_f32.append(ob)
            o.view[c.o_row0(b):c.o_row0(b) + nq, :c.D] = ob.permute(1, 0, 2).reshape(nq, c.D).to(td)
            for h in range(c.H):
                lse.view[c.lse_at(b, h):c.lse_at(b, h) + nq] = lb[h]
        return PA_OK, dict(o=o, lse=lse)

    def bwd_drop(self, d, o, d_o, lse, flags=None):
        c = d.c
        qkv = A.attn_inputs(c)["qkv"]
        td = TD[c.dt]
        g = new_out(c.T, 3 * c.D, A.PAD_DQKV, td, self.dev)
        D_ = c.D
        rk = self.rkeep_bwd(d)
        for b in range(c.B):
            N, nq, r0 = c.seq[b], c.nq_b(b), c.cu[b]
            t = self.seq3(c, qkv, b)
            q = self.queries(c, b, t, "bwd")
            k, v = self.keys(c, b, t[1], t[2], "bwd")
            do_b = from_rows(d_o.float(), c, b, "o")
            o_b = self.o_for_delta(c, o, getattr(self, "o_f32", None), b)
            P = torch.exp2(self.scores2(c, q, k) - (lse_of(lse, c, b) * torch.tensor(LOG2E, dtype=F32))[..., None])
            delta = (do_b.double() * o_b.double()).sum(-1).float()
            m = self.mask(d, b, "bwd")
            x = torch.where(m, mm(do_b, v.transpose(1, 2)) * rk, torch.zeros_like(P))
            dS = self.ds(P, x, -delta[..., None], m)
            P_lp, dS_lp = self.p_lp(torch.where(m, P, torch.zeros_like(P)), td), lp(dS, td)
            dq = mm(dS_lp, k) * torch.tensor(SCALE, dtype=F32)
            dk = mm(dS_lp.transpose(1, 2), q) * torch.tensor(LN2 if c.pre else SCALE, dtype=F32)
            dv = mm(P_lp.transpose(1, 2), do_b) * rk

            def rows(x_):
                return x_.permute(1, 0, 2).reshape(x_.shape[1], D_).to(td)
            g.view[r0:r0 + nq, :D_] = rows(dq)
            g.view[r0:r0 + N, D_:2 * D_] = rows(dk)
            g.view[r0:r0 + N, 2 * D_:3 * D_] = rows(dv)
        return PA_OK, dict(dqkv=g)


# ---- checkers --------------------------------------------------------------------------------------------------------------
def _rec(rec, group, ratio):
    if rec is not None:
        rec(group, ratio)


def check_fwd_seq(d, b, o, lse, rb, rdb, rec):
    c = d.c
    td, what = TD[c.dt], f"{d.name} seq {b}"
    tol = 8 * A.ulp32(rb["lse"].abs().clamp_min(1.0))
    _rec(rec, f"drop_lse[dt{c.dt}]", within(lse, rb["lse"], tol, what + " lse (of the UNDROPPED softmax)"))
    ref, u = rdb["o"], (U if c.dt == PA_BF16 else 0.0)
    gone = ~rdb["mask"].any(-1)                                 # every key of the row dropped: exactly 0
    assert bool((o[gone] == 0).all()), what + ": a fully dropped row is not exactly 0"
    exact = exact_regime(d.t)
    if c.fam in ("select", "pair"):
        a32 = (O_F32 + A.eps_rows(c, rb) - EPS) * rdb["A_o"]
        if exact:
            A.exact_or_bound(o, ref, a32, 0.0, c, what + " o", rec, f"drop_o_exact[dt{c.dt}]")
        else:
            _rec(rec, f"drop_o_sp[dt{c.dt}]", within(o, ref, a32 + u * rdb["A_o"] + u * ref.abs() + rdb["under"]["o"], what + " o"))
        return
    if c.fam == "uniform" and exact:
        N = c.seq[b]
        if N & (N - 1) == 0:
            equal(o, ref.float().to(td), what + " o")
        else:
            A.neighbours(o, ref, td, what + " o")
    _rec(rec, f"drop_o[dt{c.dt}]", within(o, ref, (u + EPS) * rdb["A_o"] + u * ref.abs() + rdb["under"]["o"], what + " o"))


def check_bwd_seq(d, b, dq, dk, dv, rb, rdb, rec):
    c = d.c
    what, nq = f"{d.name} seq {b}", c.nq_b(b)
    ref = dict(dq=rdb["dq"][:, :nq], dk=rdb["dk"], dv=rdb["dv"])
    got = dict(dq=dq[:, :nq], dk=dk, dv=dv)
    e = A.eps_rows(c, rb)
    K, Q, dO = rb["k"].abs(), rb["q"].abs(), rb["d_o"].abs()
    fl = rb["P"] * rdb["dabs"][..., None]                       # P . Delta: delta's error enters dS through the UNDROPPED P
    if c.fam in ("select", "pair") and exact_regime(d.t):
        aS, fl = e * rdb["dS"].abs(), O_F32 * fl
        Ab = dict(dq=SCALE * (aS @ K), dk=SCALE * (aS.transpose(1, 2) @ Q), dv=(e * rdb["PD"]).transpose(1, 2) @ dO)
        floor = dict(dq=SCALE * (fl @ K), dk=SCALE * (fl.transpose(1, 2) @ Q), dv=0.0)
        for x in ("dq", "dk", "dv"):
            A.exact_or_bound(got[x], ref[x], Ab[x], floor[x], c, f"{what} {x}", rec, f"drop_{x}_exact[dt{c.dt}]",
                             zero_exact=c.fam == "select" and not c.oshift and x != "dv")
        return
    u = U if c.dt == PA_BF16 else 0.0
    E = (u + e) * rdb["dS"].abs() + max(u, O_F32) * fl + rdb["under"]["dS"]
    bd = dict(dq=SCALE * (E @ K) + u * ref["dq"].abs() + TINY, dk=SCALE * (E.transpose(1, 2) @ Q) + u * ref["dk"].abs() + TINY,
              dv=((u + e) * rdb["PD"]).transpose(1, 2) @ dO + u * ref["dv"].abs() + rdb["under"]["dv"])
    for x in ("dq", "dk", "dv"):
        _rec(rec, f"drop_{x}[dt{c.dt}]", within(got[x], ref[x], bd[x], f"{what} {x}"))


def check_dropout(impl, d, rec=None, bwd_flags=(None,)):
    """forward, then the backward on the forward's own o and lse (select with oshift: on o + e): every buffer check of
    attention_cases, every value check above.  bwd_flags: the backward runs once per entry (extra PA_ATTN_BWD_* bits, None = the
    case's own) and every run must leave the same bits."""
    c = d.c
    assert not c.packed
    r, rd = A.reference(c), drop_reference(d)
    drop_conditions(d, r, rd)
    rc, f = impl.fwd_drop(d)
    assert rc == PA_OK, f"{d.name}: forward code {rc}"
    o, lse = A.grab_fwd(c, f)
    for b, rb in enumerate(r):
        check_fwd_seq(d, b, from_rows(o, c, b, "o"), lse_of(lse, c, b), rb, rd[b], rec)
    if not c.bwd:
        return
    if c.oshift:
        o = A.to_rows([x["o_in"].float() for x in rd], c, "o").to(TD[c.dt])
        if exact_regime(d.t):
            assert all(torch.equal(from_rows(o, c, b, "o").double(), x["o_in"]) for b, x in enumerate(rd)), "o + e is exact in the type"
    first = None
    for fl in bwd_flags:
        rc, g = impl.bwd_drop(d, o, A.attn_inputs(c)["d_o"], lse, flags=fl)
        assert rc == PA_OK, f"{d.name}: backward code {rc}"
        dd = A.grab_bwd(c, g)
        if first is None:
            first = dd
            for b, rb in enumerate(r):
                check_bwd_seq(d, b, *(from_rows(dd[:, j * c.D:(j + 1) * c.D], c, b, "tok") for j in range(3)), rb, rd[b], rec)
        else:
            same = (dd == first) | (torch.isnan(dd) & torch.isnan(first))
            assert bool(same.all()), f"{d.name}: the backward under flags {fl} differs from the first run"
