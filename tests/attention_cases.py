"""Cases, operand families, references, bounds and checkers of the exact attention parity suite (pa_attention_fwd / _bwd in the
two-pass and both single-pass forms, their packed `_varlen` forms, pa_attention_probs, pa_attention_probs_grad, pa_attention_rollout).

Used by tests/test_gpu_attention_exact.py (the HIP kernels, through the C ABI) and tests/test_attention_cases_cpu.py (the same
checkers run against `TorchAttention`, plain torch with the specified arithmetic: f32 scores, an f32 lse that is stored and read back,
P = exp2(s log2e - lse log2e), in bf16 P and dS rounded to bf16 before their products, exact f32 accumulation, ONE final rounding).
A checker hands an `impl` a case and dense CPU tensors in the C ABI's layouts and gets guarded buffers back (tests/gemm_cases.py:
guarded_in, padded, new_out, GuardedOut, SENTINEL); it neither knows nor cares where the arithmetic ran.  Imports no HIP.

Layouts (include/passt_amd.h): qkv [T][3 H 64] = [q | k | v] x head x 64 over the token rows of all sequences (T = B N, or cu_tok[B]
when packed); o / d_o [rows][H 64] with rows = token rows (every query) or b nq + q (compact prefix form); lse[(b H + h) nq + q], or
lse[h T + cu_tok[b] + q] for the packed form with every query; dqkv like qkv.  Every leading dimension is padded, each differently:
ldqkv = 3D + 8, lddqkv = 3D + 16, ldo = D + 24 (all 16-byte aligned in both types).

Operand families -- every value is a bf16 number, scale = 0.125, with and without PA_ATTN_Q_PRESCALED (the kernel then gets
q~ = round(q scale log2e) and the reference is formed from q~ / (scale log2e), the operand the kernel actually sees):

  select   keys are distinct +-8 sign codes of 64 entries, minimum pairwise Hamming distance >= 12; query q is the code of key m(q).
           The hot score is 512, every other at least 192 lower: its exponential is exactly 0 in f32.  P is one-hot, o[q] = v[m(q)],
           lse = 512, dV[k] = sum_{m(q) = k} dO[q], dQ = dK = 0.  v integers in [-8, 8], dO in {-1, 0, 1}; m differs for every
           (sequence, head): a permutation, or a many-to-one map onto key 0, key N-1 and both sides of every multiple of 32.
           `oshift`: the backward gets o + e (e in {-1, 0, 1}, sparse) instead of the forward's o -- delta = rowsum(dO o) is a
           function of the o the kernel is GIVEN, so dS = -dO.e on the hot key, dQ and dK exact integers: shows an o read with the
           wrong leading dimension, row or head, and a delta formed from anything but the stored o.
  pair     at most 128 hot key positions (0, N-1, both sides of every multiple of 32, the rest spread) carry +-4 x rows of the
           64 x 64 Hadamard matrix, all other keys are zero rows; query q is k_a + k_b of two hot keys with orthogonal codes.  Both
           hot scores are exactly 128, every other <= 0 (exponential exactly 0 in f32): P = 1/2, 1/2, o = (v_a + v_b) / 2,
           dS = +-(dP_a - dP_b) / 4.  v, dO in {-1, 0, 1}: every intermediate is a dyadic rational of at most 8 significant bits and
           dQ, dK, dV are exact in f32 accumulation (condition, asserted: every partial sum below 2^24 units).
  uniform  q = 0: P = 1/N, lse = ln N.  N a power of two: o exact; otherwise o is one of the two neighbours (in the output type) of
           the f64 value.  A key past N that is counted, or a last key that is not, moves every element.
  graded   bounded random operands (rounded to bf16) with the spike of tests/test_gpu_kernels.py::test_attention_fwd_bwd, judged per
           ELEMENT by the bounds below.

Bounds (never tuned to an implementation):
  EPS = 2^-14  the f32 exponential formed from a STORED lse: s log2e and lse log2e are at most 2^8 in magnitude, each carries an f32
               rounding of 2^-16 there, plus the rounding of lse itself and of exp2: roughly 2^-15, doubled.
  U = 2^-8     bf16, the figure of the GEMM suite: twice the unit roundoff, the factor being the margin for evaluation order.
  bf16, select / pair: torch.equal against the f64 result rounded once (o and all three thirds of dqkv, every backward form).
  f32, select / pair: where the reference has no non-zero term (and for every dQ / dK of the select family: o = v exactly there, so
               dP - delta cancels exactly) the result is exactly 0; elsewhere |got - ref| <= EPS A + floor, A the sum of the absolute
               values of the element's terms (pre-scaled q: EPS plus the score chain's term, eps_rows()), floor = 2^-21 scale (P . Delta)|K| resp. |Q| for dQ / dK (delta is formed from an o
               that carries the forward's own 2^-21; Delta = sum_d |dO o|), 0 for dV.  Forward o reads no stored lse: 2^-21 A (plus the
               score chain's term with the pre-scaled q).
  lse:         within 8 f32 ulp of max(|ref|, 1), per query.
  graded:      o   (U + EPS) (P |V|) + U |o|                dV  (U + EPS) (P^T |dO|) + U |dV|
               E_S = (U + EPS) |dS| + U P . Delta           (Delta: O is read back in bf16 for delta)
               dQ  scale (E_S |K|) + U |dQ|                 dK  scale (E_S^T |Q|) + U |dK|          f32: U = 0, except that
               E_S keeps 2^-21 P . Delta, the floor of the exact families: on a row whose P is one-hot (the spike) dP - delta cancels
               to 1e-20 of dP, and ANY f32 evaluation leaves 2^-24 (|dP| + |delta|) there -- the specified plain-torch arithmetic
               misses EPS |dS| alone by a factor of up to 8951 on that row (profiles/attention_exact_parity.txt).
"""
import functools
import math
from dataclasses import dataclass, replace

import torch

from tests.gemm_cases import (PA_BF16, PA_EINVAL, PA_EUNSUPPORTED, PA_F32, PA_OK, SENTINEL, TD, GuardedOut, equal, guarded_in,  # noqa: F401
                              new_out, padded, within)

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
HD = 64
SCALE = 0.125
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
SL2 = SCALE * LOG2E
PRE, TWO_PASS, SINGLE_PASS, SINGLE_PASS_W16 = 1, 2, 4, 8
FK = 512                              # the single pass holds at most this many keys
EPS, U = 2.0 ** -14, 2.0 ** -8
O_F32 = 2.0 ** -21
PAD_QKV, PAD_DQKV, PAD_O = 8, 16, 24
# the bounds of tests/test_gpu_kernels.py::test_attention_fwd_bwd in bf16: max|got - ref| / max|ref| per call
OLD_O, OLD_D = 1.5e-2, 4e-2
PGRAD_GRAD, PGRAD_CAM = 0, 1
ROLLOUT_ATTN, ROLLOUT_CAM = 0, 1
NR = 2                                # row vectors per sequence of the rollout cases
G_SCALE = 0.25

N_PAIR_FORMS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193, 255, 257, 511, 512, 513, 1190)     # forward and the kernel pair
N_SINGLE = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 479, 480, 481, 511, 512)          # both single-pass forms, the library's choice
BHS = ((1, 1), (1, 7), (2, 4), (3, 3), (17, 1), (1, 12))
LIBRARY_SINGLE_N = (33,)              # with (B, H) = (64, 8) on top: pa_attention_bwd picks the single pass itself from B H = 512
NQ_N = (33, 130, 257)
NQS = (1, 2, 31, 32, 33, 127, 128, 129)
PACKED = ((1, 33, 2, 129, 64, 1), (300, 1), (65, 128, 32), (257,), (33, 1, 65))       # the last: a length-1 sequence in the middle
FAMILIES = ("select", "pair", "uniform", "graded")
CODE_SEED, NCODES, MIN_HAMMING = 0, 1280, 12


@dataclass(frozen=True)
class AC:
    """one forward (+ backward) problem.  flags: PRE | one of the backward forms.  nq: 0 = every query.  lens: packed lengths
    (B and N are then len(lens) and max(lens)).  many: the select family's many-to-one map.  bwd: run the backward."""
    dt: int
    B: int
    H: int
    N: int
    fam: str
    flags: int = 0
    nq: int = 0
    lens: tuple = ()
    many: bool = False
    oshift: bool = False
    bwd: bool = True
    seed: int = 0

    @property
    def name(self):
        s = f"{self.fam},dt{self.dt},B{self.B}H{self.H}N{self.N},flags{self.flags}"
        s += f",nq{self.nq}" if self.nq else ""
        s += f",lens{list(self.lens)}" if self.lens else ""
        return s + (",many" if self.many else "") + (",oshift" if self.oshift else "")

    @property
    def pre(self):
        return bool(self.flags & PRE)

    @property
    def packed(self):
        return bool(self.lens)

    @property
    def D(self):
        return self.H * HD

    @property
    def seq(self):
        return tuple(self.lens) if self.lens else (self.N,) * self.B

    @property
    def cu(self):
        out = [0]
        for n in self.seq:
            out.append(out[-1] + n)
        return out

    @property
    def T(self):
        return self.cu[-1]

    @property
    def nqk(self):
        """the kernels' nq: N (max N when packed) means every query"""
        return self.N if (self.nq == 0 or self.nq >= self.N) else self.nq

    @property
    def all_q(self):
        return self.nqk == self.N

    def nq_b(self, b):
        return min(self.nqk, self.seq[b])

    @property
    def o_rows(self):
        return self.T if (self.packed and self.all_q) else self.B * self.nqk

    def o_row0(self, b):
        return self.cu[b] if (self.packed and self.all_q) else b * self.nqk

    @property
    def n_lse(self):
        return self.H * self.o_rows

    def lse_at(self, b, h):
        return h * self.T + self.cu[b] if (self.packed and self.all_q) else (b * self.H + h) * self.nqk

    @property
    def single_pass(self):
        """pa_attention_bwd runs this case as the single kernel (the library's own choice takes it from B H >= 512)"""
        can = self.dt == PA_BF16 and self.pre and not self.packed and self.all_q and self.N <= FK
        return can and not (self.flags & TWO_PASS) and (bool(self.flags & (SINGLE_PASS | SINGLE_PASS_W16)) or self.B * self.H >= 512)


def bwd_form(c):
    if c.single_pass:
        return "single_w16" if c.flags & SINGLE_PASS_W16 else "single"
    return "packed" if c.packed else "two_pass"


# ---- case lists ----------------------------------------------------------------------------------------------------------
def bh_of(j, N):
    return (1, 1) if N > 600 else BHS[j % len(BHS)]


def _family_cases(dt, B, H, N, flags, j, **kw):
    out = [AC(dt, B, H, N, "select", flags, many=bool(j & 1), seed=j, **kw),
           AC(dt, B, H, N, "select", flags, many=not (j & 1), oshift=True, seed=j + 1, **kw),
           AC(dt, B, H, N, "uniform", flags, seed=j, **kw), AC(dt, B, H, N, "graded", flags, seed=j, **kw)]
    if N >= 2:
        out.append(AC(dt, B, H, N, "pair", flags, seed=j, **kw))
    return out


def pair_form_cases(N):
    """forward and the dQ + dK/dV kernel pair at one N: both types, with and without the pre-scaled q, every family; two (B, H)"""
    j = N_PAIR_FORMS.index(N)
    out = []
    for d, (B, H) in enumerate((bh_of(j, N), bh_of(j + 3, N))):
        for dt in (PA_F32, PA_BF16):
            for pre in (0, PRE):
                out += _family_cases(dt, B, H, N, pre | (TWO_PASS if (dt == PA_BF16 and pre) else 0), j + d)
        if N > 600:
            break
    return out


def single_cases(N):
    """bf16, pre-scaled q: the single pass in both forms and the library's own choice"""
    j = N_SINGLE.index(N)
    out = []
    for d, form in enumerate((SINGLE_PASS, SINGLE_PASS_W16, 0)):
        B, H = bh_of(j + 2 * d + 1, N)
        out += _family_cases(PA_BF16, B, H, N, PRE | form, j + d)
    if N in LIBRARY_SINGLE_N:                                   # B H = 512: the library's own choice IS the single pass
        out += [c for c in _family_cases(PA_BF16, 64, 8, N, PRE, j + 3) if c.fam in ("select", "pair") and not c.oshift]
    return out


def prefix_cases(N):
    out = []
    for j, nq in enumerate(q for q in NQS + (N - 1,) if q < N):
        B, H = BHS[(j + N) % len(BHS)]
        for dt in (PA_F32, PA_BF16):
            pre = PRE if (j + dt) & 1 else 0
            out += _family_cases(dt, B, H, N, pre, j, nq=nq)
    return out


def packed_cases(lens):
    out = []
    for j, nq in enumerate((0, 2)):
        for dt in (PA_F32, PA_BF16):
            for pre in (0, PRE):
                H = (3, 1, 7, 2, 3)[PACKED.index(lens)]
                out += _family_cases(dt, len(lens), H, max(lens), pre, j + len(lens), nq=nq, lens=tuple(lens))
    return out


def all_cases():
    out = []
    for N in N_PAIR_FORMS:
        out += pair_form_cases(N)
    for N in N_SINGLE:
        out += single_cases(N)
    for N in NQ_N:
        out += prefix_cases(N)
    for lens in PACKED:
        out += packed_cases(lens)
    return out


# ---- operands ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def sign_codes():
    g = torch.Generator().manual_seed(CODE_SEED)
    return (torch.randint(0, 2, (NCODES, HD), generator=g) * 2 - 1).float()


def min_hamming(codes):
    d = (HD - codes.double() @ codes.double().t()) / 2
    d.fill_diagonal_(HD)
    return int(d.min())


@functools.lru_cache(maxsize=1)
def hadamard():
    h = torch.ones(1, 1)
    while h.shape[0] < HD:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def edge_positions(N):
    """0, N-1 and the keys on either side of every multiple of 32 (the 32-key blocks, 64-key tiles and 128-row blocks all end there)"""
    s = {0, N - 1}
    for t in range(32, N, 32):
        s |= {t - 1, t}
    return sorted(s)


def hot_positions(N):
    s = edge_positions(N)
    assert len(s) <= 128
    want = min(N, 128)
    if len(s) < want:
        rest = [p for p in range(N) if p not in set(s)]
        step = len(rest) / (want - len(s))
        s = sorted(set(s) | {rest[int(i * step)] for i in range(want - len(s))})
    return s


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def select_map(N, many, g, bh):
    if not many:
        return torch.randperm(N, generator=g)
    t = torch.tensor(edge_positions(N))
    return t[(torch.arange(N) * 7 + bh) % len(t)]


def _pair_code(ci):
    return (1.0 if ci < 64 else -1.0) * 4.0 * hadamard()[ci % 64]


def _seq_operands(c, b):
    """q, k, v [H][N_b][64] (q unscaled), dO [H][nq_b][64], and the family's own bookkeeping"""
    N, H, nq = c.seq[b], c.H, c.nq_b(b)
    g = torch.Generator().manual_seed(7919 * c.seed + 131 * b + N)
    q, k, v = torch.zeros(H, N, HD), torch.zeros(H, N, HD), torch.zeros(H, N, HD)
    info = {}
    if c.fam == "select":
        codes, maps = sign_codes(), []
        for h in range(H):
            bh = b * H + h
            k[h] = 8 * codes[(torch.arange(N) + 37 * bh + 11 * b) % NCODES]
            maps.append(select_map(N, c.many, g, bh))
            q[h] = k[h][maps[-1]]
        v, d_o = _ints(g, -8, 8, H, N, HD), _ints(g, -1, 1, H, nq, HD)
        info["map"] = torch.stack(maps)
        if c.oshift:
            info["e"] = _ints(g, -1, 1, H, nq, HD) * (torch.rand(H, nq, HD, generator=g) < 0.1)
    elif c.fam == "pair":
        hot = hot_positions(N)
        nh = len(hot)
        pa, pb = torch.zeros(H, N, dtype=torch.long), torch.zeros(H, N, dtype=torch.long)
        for h in range(H):
            bh = b * H + h
            ci = [(i + 5 * bh) % 128 for i in range(nh)]
            for i, p in enumerate(hot):
                k[h, p] = _pair_code(ci[i])
            for t in range(N):
                if nh == 1:
                    q[h, t], pa[h, t], pb[h, t] = 2 * k[h, hot[0]], hot[0], hot[0]
                    continue
                ia = (t + bh) % nh
                ib = (ia + 1 + (t // nh) % (nh - 1)) % nh
                while ib == ia or ci[ia] % 64 == ci[ib] % 64:
                    ib = (ib + 1) % nh
                q[h, t], pa[h, t], pb[h, t] = k[h, hot[ia]] + k[h, hot[ib]], hot[ia], hot[ib]
        v, d_o = _ints(g, -1, 1, H, N, HD), _ints(g, -1, 1, H, nq, HD)
        info.update(a=pa, b=pb, hot=hot)
    elif c.fam == "uniform":
        k, v, d_o = _ints(g, -8, 8, H, N, HD), _ints(g, -8, 8, H, N, HD), _ints(g, -1, 1, H, nq, HD)
    else:
        x = ((torch.rand(3, H, N, HD, generator=g) * 2 - 1) * 1.5)
        if N > 70 and b == 0:                                   # the online-softmax maximum jumps mid-sequence
            x[0, 0, N - 3] *= 4.0
            x[1, 0, 69] = x[0, 0, N - 3]
        q, k, v = (t.to(BF16).float() for t in x)
        d_o = (torch.rand(H, nq, HD, generator=g) * 2 - 1).to(BF16).float()
    return q, k, v, d_o, info


def to_rows(per_seq, c, kind):
    """per-sequence [H][n][64] tensors -> the dense [rows][H 64] layout.  kind: tok (qkv's rows) | o (o / d_o rows; rows nobody owns: NaN)"""
    rows = c.T if kind == "tok" else c.o_rows
    out = torch.full((rows, c.D), float("nan"))
    for b, t in enumerate(per_seq):
        r0 = c.cu[b] if kind == "tok" else c.o_row0(b)
        out[r0:r0 + t.shape[1]] = t.permute(1, 0, 2).reshape(t.shape[1], c.D)
    return out


def from_rows(dense, c, b, kind, n=None):
    """[rows][H 64] -> sequence b's [H][n][64]"""
    r0 = c.cu[b] if kind == "tok" else c.o_row0(b)
    n = (c.seq[b] if kind == "tok" else c.nq_b(b)) if n is None else n
    return dense[r0:r0 + n].reshape(n, c.H, HD).permute(1, 0, 2)


def lse_of(flat, c, b):
    """flat lse -> sequence b's [H][nq_b]"""
    return torch.stack([flat[c.lse_at(b, h):c.lse_at(b, h) + c.nq_b(b)] for h in range(c.H)])


def map_offsets(c, head_mean):
    """float offset of every sequence's [Ho][nq_b][N_b] block in the output of pa_attention_probs / _probs_grad (fixed: the header's
    out[((b Ho + h) nq + q) N + k] is the same thing)"""
    Ho, off = (1 if head_mean else c.H), [0]
    for b in range(c.B):
        off.append(off[-1] + Ho * c.nq_b(b) * c.seq[b])
    return off


def do_compact(c):
    """d_o as the sibling entries read it: the compact prefix form, or qkv's token rows"""
    return int(not c.all_q)


def _key(c):
    return replace(c, flags=c.flags & PRE, bwd=True)


@functools.lru_cache(maxsize=6)
def _inputs(c):
    td = TD[c.dt]
    seqs = [_seq_operands(c, b) for b in range(c.B)]
    q = to_rows([s[0] for s in seqs], c, "tok")
    k = to_rows([s[1] for s in seqs], c, "tok")
    v = to_rows([s[2] for s in seqs], c, "tok")
    for t in (q, k, v):
        assert torch.equal(t.to(BF16).float(), t), "every operand is a bf16 number"
    qs = (q * torch.tensor(SL2, dtype=F32)).to(td) if c.pre else q.to(td)
    qkv = torch.cat([qs, k.to(td), v.to(td)], 1)
    # the operand the kernel sees; the reference reads it as qs * qfac (pre-scaled: q~ / (scale log2e)) and applies the factor AFTER
    # every sum, so sums of exact products stay exact in f64 and terms that cancel give exactly 0
    qref, qfac = qs.double(), (1 / SL2 if c.pre else 1.0)
    d_o = to_rows([s[3] for s in seqs], c, "o").to(td)
    return dict(qkv=qkv, d_o=d_o, qref=qref, qfac=qfac, k=k.double(), v=v.double(), info=[s[4] for s in seqs])


def attn_inputs(c):
    return _inputs(_key(c))


# ---- f64 reference -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=6)
def _reference(c):
    i = _inputs(c)
    out = []
    for b in range(c.B):
        nq = c.nq_b(b)
        q, k, v = (from_rows(t, c, b, "tok") for t in (i["qref"], i["k"], i["v"]))
        d_o = from_rows(i["d_o"].double(), c, b, "o")
        qq = q[:, :nq]
        fac = SCALE * i["qfac"]
        s = (qq @ k.transpose(1, 2)) * fac
        mx = s.max(-1, keepdim=True).values
        P = torch.exp(s - mx)
        if c.fam in ("select", "pair"):
            # the families' condition: every cold exponential is exactly 0 in f32 (below e^-128 here: no bound could see it), and
            # the hot ones are exp(0) = 1, so P is exactly one-hot resp. 1/2, 1/2 and every product below is exact in f64
            P = torch.where(P < 2.0 ** -126, torch.zeros_like(P), P)
        l = P.sum(-1, keepdim=True)
        lse = mx[..., 0] + torch.log(l[..., 0])
        o = (P @ v) / l                                         # one division after the sum: exact sums stay exact (uniform: sum v / N)
        P = P / l
        o_in = o
        if c.oshift:
            o_in = o + i["info"][b]["e"].double()
        dP = d_o @ v.transpose(1, 2)
        delta = (d_o * o_in).sum(-1)
        dabs = (d_o * o_in).abs().sum(-1)
        dS = P * (dP - delta[..., None])
        dq = torch.zeros_like(q)
        dq[:, :nq] = SCALE * (dS @ k)
        r = dict(P=P, lse=lse, o=o, o_in=o_in, dS=dS, dabs=dabs, dq=dq, dk=fac * (dS.transpose(1, 2) @ qq), dv=P.transpose(1, 2) @ d_o,
                 A_o=P @ v.abs(), A_dv=P.transpose(1, 2) @ d_o.abs(), s=s, q=qq * i["qfac"], k=k, v=v, d_o=d_o, dP=dP)
        out.append(r)
    return out


def reference(c):
    return _reference(_key(c))


def conditions(c, i, r):
    """the conditions under which a family is exact, per case (never clipped)"""
    for b, rb in enumerate(r):
        s, N = rb["s"], c.seq[b]
        if c.fam == "select":
            m = i["info"][b]["map"][:, :c.nq_b(b)]
            hot = s.gather(2, m[..., None])[..., 0]
            assert float((hot - 512).abs().max()) <= 512 * 2.0 ** -8, "hot score 512 (pre-scaled: times 1 + 2^-9 at most)"
            cold = s.scatter(2, m[..., None], -1e30)
            if N > 1:
                assert float((hot - cold.max(-1).values).min()) >= 191, "every other score at least 192 lower"
            for h in range(c.H):
                cs = torch.zeros(N, HD, dtype=F64).index_add_(0, m[h], rb["d_o"][h])
                assert float(cs.abs().max()) <= 256, "bf16 holds every column sum of dO"
        elif c.fam == "pair" and N >= 2:
            pa, pb = (i["info"][b][x][:, :c.nq_b(b)] for x in "ab")
            sa, sb = s.gather(2, pa[..., None]), s.gather(2, pb[..., None])
            assert bool((sa == sb).all()) and float((sa - 128).abs().max()) <= 128 * 2.0 ** -8 and bool((pa != pb).all())
            cold = s.scatter(2, pa[..., None], -1e30).scatter(2, pb[..., None], -1e30)
            assert float(cold.max()) <= 0 or N == 2, "every other score <= 0"
            # exact f32 accumulation: sums of at most N terms, each a multiple of 2^-4 below 2^8
            assert N * 2 ** 8 * 2 ** 4 < 2 ** 24
        elif c.fam == "uniform":
            assert float(rb["q"].abs().max()) == 0


# ---- plain torch with the specified arithmetic ---------------------------------------------------------------------------
def mm(a, b):
    """f32 x f32 -> f32 with exact accumulation, one rounding"""
    return (a.double() @ b.double()).float()


def lp(x, td):
    return x.to(td).float()


class TorchAttention:
    """The entries in plain torch on the CPU, in the kernels' calling conventions.  The small methods are the places an attention
    kernel goes wrong; the fault models of tests/test_attention_cases_cpu.py override them one at a time."""
    name = "torch"
    dev = "cpu"

    # -- hooks
    def n_keys(self, c, b, phase):
        return c.seq[b]

    def keys(self, c, b, k, v, phase):
        n = self.n_keys(c, b, phase)
        return k[:, :n], v[:, :n]

    def queries(self, c, b, qkv3, phase):
        """[H][nq_b][64] as stored"""
        return qkv3[0][:, :c.nq_b(b)]

    def p_lp(self, P, td):
        return lp(P, td)

    def o_for_delta(self, c, o_dense, o_f32, b):
        return from_rows(o_dense.float(), c, b, "o")

    def dv_rows(self, c, b):
        return c.seq[b]

    # -- arithmetic
    def scores2(self, c, q, k):
        """scores in log2 units, f32"""
        s = mm(q, k.transpose(1, 2))
        return s if c.pre else (s * torch.tensor(SCALE, dtype=F32)) * torch.tensor(LOG2E, dtype=F32)

    def seq3(self, c, qkv, b):
        N = c.seq[b]
        return qkv[c.cu[b]:c.cu[b] + N].float().reshape(N, 3, c.H, HD).permute(1, 2, 0, 3)

    def fwd_seq(self, c, qkv, b):
        td = TD[c.dt]
        t = self.seq3(c, qkv, b)
        q = self.queries(c, b, t, "fwd")
        k, v = self.keys(c, b, t[1], t[2], "fwd")
        s2 = self.scores2(c, q, k)
        m = s2.max(-1, keepdim=True).values
        # the forward reads no stored lse: p = exp2(s - max), the row sum of the f32 p, one division at the end
        p = torch.exp2(s2 - m)
        l = p.double().sum(-1, keepdim=True).float()
        lse = ((m + torch.log2(l)) * torch.tensor(LN2, dtype=F32))[..., 0]
        return mm(self.p_lp(p, td), v) / l, lse

    def fwd(self, c, qkv):
        td = TD[c.dt]
        o = new_out(c.o_rows, c.D, PAD_O, td, self.dev)
        lse = GuardedOut(c.n_lse, F32, self.dev)
        self.o_f32 = []
        for b in range(c.B):
            ob, lb = self.fwd_seq(c, qkv, b)
            nq = c.nq_b(b)
            self.o_f32.append(ob)
            o.view[c.o_row0(b):c.o_row0(b) + nq, :c.D] = ob.permute(1, 0, 2).reshape(nq, c.D).to(td)
            for h in range(c.H):
                lse.view[c.lse_at(b, h):c.lse_at(b, h) + nq] = lb[h]
        return PA_OK, dict(o=o, lse=lse)

    def bwd(self, c, qkv, o, d_o, lse):
        td = TD[c.dt]
        g = new_out(c.T, 3 * c.D, PAD_DQKV, td, self.dev)
        D = c.D
        for b in range(c.B):
            N, nq, r0 = c.seq[b], c.nq_b(b), c.cu[b]
            t = self.seq3(c, qkv, b)
            q = self.queries(c, b, t, "bwd")
            k, v = self.keys(c, b, t[1], t[2], "bwd")
            nk = k.shape[1]
            do_b = from_rows(d_o.float(), c, b, "o")
            o_b = self.o_for_delta(c, o, getattr(self, "o_f32", None), b)
            P = torch.exp2(self.scores2(c, q, k) - (lse_of(lse, c, b) * torch.tensor(LOG2E, dtype=F32))[..., None])
            delta = (do_b.double() * o_b.double()).sum(-1).float()
            dS = P * (mm(do_b, v.transpose(1, 2)) - delta[..., None])
            P_lp, dS_lp = self.p_lp(P, td), lp(dS, td)
            dq = mm(dS_lp, k) * torch.tensor(SCALE, dtype=F32)
            dk = mm(dS_lp.transpose(1, 2), q) * torch.tensor(LN2 if c.pre else SCALE, dtype=F32)
            dv = mm(P_lp.transpose(1, 2), do_b)

            def rows(x):
                return x.permute(1, 0, 2).reshape(x.shape[1], D).to(td)
            g.view[r0:r0 + nq, :D] = rows(dq)
            if c.packed and nq < N:
                g.view[r0 + nq:r0 + N, :D] = 0
            nk = min(nk, N)
            g.view[r0:r0 + nk, D:2 * D] = rows(dk)[:nk]
            nv = min(nk, self.dv_rows(c, b))
            g.view[r0:r0 + nv, 2 * D:3 * D] = rows(dv)[:nv]
        return PA_OK, dict(dqkv=g)


    # -- the sibling entries
    def probs_seq(self, c, qkv, lse, b):
        t = self.seq3(c, qkv, b)
        k, _ = self.keys(c, b, t[1], t[2], "probs")
        return torch.exp2(self.scores2(c, self.queries(c, b, t, "probs"), k) - (lse_of(lse, c, b) * torch.tensor(LOG2E, dtype=F32))[..., None])

    def grad_seq(self, c, qkv, d_o, b):
        return mm(from_rows(d_o.float(), c, b, "o"), self.seq3(c, qkv, b)[2].transpose(1, 2))

    def probs(self, c, qkv, lse, head_mean, d_o=None, mode=None):
        """pa_attention_probs (mode None) / pa_attention_probs_grad"""
        off = map_offsets(c, head_mean)
        g = GuardedOut(off[-1], F32, self.dev)
        for b in range(c.B):
            if mode is None:
                x = self.probs_seq(c, qkv, lse, b)
            elif mode == PGRAD_GRAD:
                x = self.grad_seq(c, qkv, d_o, b)
            else:
                x = (self.probs_seq(c, qkv, lse, b) * self.grad_seq(c, qkv, d_o, b)).clamp_min(0)
            if head_mean:
                x = x.double().sum(0, keepdim=True).float() * torch.tensor(1.0 / c.H, dtype=F32)
            g.view[off[b]:off[b + 1]] = x.reshape(-1)
        return PA_OK, g

    def rollout(self, c, qkv, lse, d_o, r_in, mode, slices, a, b_, g_scale):
        g = GuardedOut(NR * c.T, F32, self.dev)
        for b in range(c.B):
            N, nq = c.seq[b], c.nq_b(b)
            M = self.probs_seq(c, qkv, lse, b)
            if mode == ROLLOUT_CAM:
                M = (M * (self.grad_seq(c, qkv, d_o, b) * torch.tensor(g_scale, dtype=F32))).clamp_min(0)
            M = M.double().sum(0).float() * torch.tensor(1.0 / c.H, dtype=F32)
            r = r_in[NR * c.cu[b]:NR * c.cu[b + 1]].view(NR, N)
            g.view[NR * c.cu[b]:NR * c.cu[b + 1]] = (a * r + b_ * mm(r[:, :nq], M)).reshape(-1)
        return PA_OK, g


# ---- buffers -------------------------------------------------------------------------------------------------------------
def _buffer(g, what, N):
    buf = g.buf.cpu()
    assert bool((buf[:g.lo] == SENTINEL).all()), f"{what}: a write in front of the output"
    assert bool((buf[g.lo + g.n:] == SENTINEL).all()), f"{what}: a write behind the output"
    full = buf[g.lo:g.lo + g.n].view(g.view.shape)
    if full.dim() == 2:
        assert bool((full[:, N:] == SENTINEL).all()), f"{what}: a write into the gap columns"
        return full[:, :N].clone()
    return full.clone()


def _owned(dense, mask, what):
    """every promised element written, no other"""
    assert not bool((dense[mask] == SENTINEL).any()), f"{what}: elements the kernel never wrote"
    assert bool((dense[~mask] == SENTINEL).all()), f"{what}: a write into elements the header says are not written"
    assert not bool(torch.isnan(dense[mask].float()).any()), f"{what}: NaN (a guard was read)"


def grab_fwd(c, f):
    """dense o [o_rows][D] and flat lse after every buffer check (rows / entries nobody owns: NaN)"""
    o, lse = _buffer(f["o"], c.name + " o", c.D), _buffer(f["lse"], c.name + " lse", 0)
    mo, ml = torch.zeros(c.o_rows, dtype=torch.bool), torch.zeros(c.n_lse, dtype=torch.bool)
    for b in range(c.B):
        mo[c.o_row0(b):c.o_row0(b) + c.nq_b(b)] = True
        for h in range(c.H):
            ml[c.lse_at(b, h):c.lse_at(b, h) + c.nq_b(b)] = True
    _owned(o, mo[:, None].expand_as(o), c.name + " o")
    _owned(lse, ml, c.name + " lse")
    o[~mo] = float("nan")
    lse[~ml] = float("nan")
    return o, lse


def grab_bwd(c, g):
    """dense dqkv [T][3D]: the K and V thirds of every row written, the Q third of rows q >= nq left alone (fixed) / zero (packed)"""
    d = _buffer(g["dqkv"], c.name + " dqkv", 3 * c.D)
    m = torch.ones(c.T, 3 * c.D, dtype=torch.bool)
    for b in range(c.B):
        if not c.packed:
            m[c.cu[b] + c.nq_b(b):c.cu[b + 1], :c.D] = False
    _owned(d, m, c.name + " dqkv")
    return d


# ---- checkers ------------------------------------------------------------------------------------------------------------
def _rec(rec, group, ratio):
    if rec is not None:
        rec(group, ratio)


def ulp32(x):
    return 2.0 ** (torch.floor(torch.log2(x)) - 23)


def neighbours(got, ref, td, what):
    """got is one of the two numbers of `td` that enclose the f64 value (the value itself where it is one)"""
    it = torch.int16 if td == BF16 else torch.int32
    n = ref.to(F32).to(td) if td == BF16 else ref.to(td)
    away = ref.abs() > n.double().abs()
    other = (n.contiguous().view(it) + torch.where(away, 1, -1).to(it)).view(td)
    other = torch.where(n.double() == ref, n, other)
    ok = (got == n) | (got == other)
    assert bool(ok.all()), (what, "not a neighbour of the f64 value:", int((~ok).sum()), "of", ok.numel())


def exact_or_bound(got, ref, A, floor, c, what, rec, group, zero_exact=False):
    """select / pair.  bf16: torch.equal against the f64 result rounded once.  f32: exactly 0 where no term is (zero_exact: wherever the
    reference is 0), EPS A + floor elsewhere"""
    if c.dt == PA_BF16:
        equal(got, ref.float().to(BF16), what)
        return
    bound = A + floor
    if zero_exact:
        bound = torch.where(ref == 0, torch.zeros_like(bound), bound)
    z = bound == 0
    assert bool((got[z] == 0).all()), (what, "not exactly 0 where the reference has no term:", int((got[z] != 0).sum()))
    _rec(rec, group, within(got, ref, bound, what))


def check_fwd_seq(c, b, o, lse, rb, rec):
    td, what = TD[c.dt], f"{c.name} seq {b}"
    tol = 8 * ulp32(rb["lse"].abs().clamp_min(1.0))
    _rec(rec, f"lse[dt{c.dt}]", within(lse, rb["lse"], tol, what + " lse"))
    ref = rb["o"]
    if c.fam in ("select", "pair"):
        # pre-scaled q: the forward's score chain starts from C = -(running maximum) (attention.hip, attn_fwd_body), the same
        # rounding point as in the backward (eps_rows): two hot keys of one row then differ by that much
        exact_or_bound(o, ref, (O_F32 + eps_rows(c, rb) - EPS) * rb["A_o"], 0.0, c, what + " o", rec, f"o_exact[dt{c.dt}]")
    elif c.fam == "uniform":
        N = c.seq[b]
        if N & (N - 1) == 0:
            equal(o, ref.float().to(td), what + " o")
        else:
            neighbours(o, ref, td, what + " o")
    if c.fam in ("graded", "uniform"):
        u = U if c.dt == PA_BF16 else 0.0
        _rec(rec, f"o[dt{c.dt}]", within(o, ref, (u + EPS) * rb["A_o"] + u * ref.abs(), what + " o"))


def eps_rows(c, rb):
    """EPS per query row [H][nq][1], plus the score chain's own term where q is pre-scaled: attention.hip then starts the chain of
    matrix products from C = -lse log2e (attn_bwd_dq / dkdv / fused: "score - row reference straight from the matrix pipe"), so each of
    its STEPS accumulations (f32: 32 products of depth 2, bf16: 4 of depth 16) rounds a partial sum of magnitude up to
    |lse log2e| + sum_d |q~ k| to f32: the exponent is off by at most STEPS 2^-24 of that, the probability by ln 2 times as much.
    (Without the flag the chain starts from 0 and one fma subtracts lse log2e: inside EPS.)  Proportional to the row's own scores:
    2e-3 for the select family's 512, 3e-4 for the pair family's 128, below EPS for bounded random rows."""
    if not c.pre:
        return torch.full((*rb["lse"].shape, 1), EPS, dtype=F64)
    steps = 32 if c.dt == PA_F32 else 4
    mag = LOG2E * (rb["lse"].abs() + SCALE * (rb["q"].abs() @ rb["k"].abs().transpose(1, 2)).max(-1).values)
    return (EPS + LN2 * steps * 2.0 ** -24 * mag)[..., None]


def graded_bounds(c, rb):
    u = U if c.dt == PA_BF16 else 0.0
    e = u + eps_rows(c, rb)
    E = e * rb["dS"].abs() + max(u, O_F32) * rb["P"] * rb["dabs"][..., None]
    return dict(dq=SCALE * (E @ rb["k"].abs()) + u * rb["dq"][:, :E.shape[1]].abs(),
                dk=SCALE * (E.transpose(1, 2) @ rb["q"].abs()) + u * rb["dk"].abs(),
                dv=(e * rb["P"]).transpose(1, 2) @ rb["d_o"].abs() + u * rb["dv"].abs())


def check_bwd_seq(c, b, dq, dk, dv, rb, rec):
    what, nq, form = f"{c.name} seq {b}", c.nq_b(b), bwd_form(c)
    ref = dict(dq=rb["dq"][:, :nq], dk=rb["dk"], dv=rb["dv"])
    got = dict(dq=dq[:, :nq], dk=dk, dv=dv)
    if c.packed and nq < c.seq[b]:
        assert bool((dq[:, nq:] == 0).all()), what + ": the Q third of rows q >= nq is written as zero"
    if c.fam in ("select", "pair"):
        e = eps_rows(c, rb)
        aS, fl = e * rb["dS"].abs(), O_F32 * rb["P"] * rb["dabs"][..., None]
        A = dict(dq=SCALE * (aS @ rb["k"].abs()), dk=SCALE * (aS.transpose(1, 2) @ rb["q"].abs()),
                 dv=(e * rb["P"]).transpose(1, 2) @ rb["d_o"].abs())
        floor = dict(dq=SCALE * (fl @ rb["k"].abs()), dk=SCALE * (fl.transpose(1, 2) @ rb["q"].abs()), dv=0.0)
        for x in ("dq", "dk", "dv"):
            exact_or_bound(got[x], ref[x], A[x], floor[x], c, f"{what} {x}", rec, f"{x}_exact[{form},dt{c.dt}]",
                           zero_exact=c.fam == "select" and not c.oshift and x != "dv")
    else:
        bd = graded_bounds(c, rb)
        for x in ("dq", "dk", "dv"):
            _rec(rec, f"{x}[{form},dt{c.dt}]", within(got[x], ref[x], bd[x], f"{what} {x}"))


def check_attention(impl, c, rec=None):
    """forward, then the backward on the forward's own o and lse (select with oshift: on o + e): every buffer check, every value check"""
    i, r = attn_inputs(c), reference(c)
    conditions(c, i, r)
    rc, f = impl.fwd(c, i["qkv"])
    assert rc == PA_OK, f"{c.name}: forward code {rc}"
    o, lse = grab_fwd(c, f)
    for b, rb in enumerate(r):
        check_fwd_seq(c, b, from_rows(o, c, b, "o"), lse_of(lse, c, b), rb, rec)
    if not c.bwd:
        return
    if c.oshift:
        o = to_rows([rb["o_in"].float() for rb in r], c, "o").to(TD[c.dt])
        assert all(torch.equal(from_rows(o, c, b, "o").double(), rb["o_in"]) for b, rb in enumerate(r)), "o + e is exact in the type"
    rc, g = impl.bwd(c, i["qkv"], o, i["d_o"], lse)
    assert rc == PA_OK, f"{c.name}: backward code {rc}"
    d = grab_bwd(c, g)
    D = c.D
    for b, rb in enumerate(r):
        check_bwd_seq(c, b, *(from_rows(d[:, j * D:(j + 1) * D], c, b, "tok") for j in range(3)), rb, rec)


def old_metric_passes(c, o, d):
    """would max|got - ref| / max|ref| per call, the bound of test_attention_fwd_bwd, accept these dense results?"""
    r = reference(c)

    def rel(g, x):
        g = torch.nan_to_num(g.double(), nan=0.0)
        return float((g - x).abs().max() / (x.abs().max() + 1e-30))
    ro = to_rows([rb["o"] for rb in r], c, "o")
    rd = [to_rows([rb[x] for rb in r], c, "tok") for x in ("dq", "dk", "dv")]
    D = c.D
    lim_o, lim_d = (OLD_O, OLD_D) if c.dt == PA_BF16 else (2e-5, 5e-5)
    return rel(o, torch.nan_to_num(ro, nan=0.0)) < lim_o and all(rel(d[:, j * D:(j + 1) * D], rd[j]) < lim_d for j in range(3))


# ---- the sibling entries, on the select and pair families ------------------------------------------------------------------
def sibling_cases():
    out, j = [], 0
    for N in (1, 33, 64, 65, 129, 257):
        for fam in ("select", "pair"):
            for dt in (PA_F32, PA_BF16):
                j += 1
                if fam == "pair" and N < 2:
                    continue
                B, H = BHS[j % len(BHS)]
                out.append(AC(dt, B, H, N, fam, flags=PRE * (j // 2 & 1), nq=(0, 2, 33)[j % 3] if N > 33 else 0, many=bool(j & 1), seed=j, bwd=False))
    for j, lens in enumerate(PACKED[:2]):
        for fam in ("select", "pair"):
            for dt in (PA_F32, PA_BF16):
                out.append(AC(dt, len(lens), 3, max(lens), fam, flags=PRE * (dt == PA_BF16), nq=2 * (fam == "pair"), lens=lens, seed=j, bwd=False))
    return out


def ref_lse(c, r):
    """the f64 lse rounded to f32 in the layout the forward leaves (entries nobody owns: NaN)"""
    lse = torch.full((c.n_lse,), float("nan"))
    for b, rb in enumerate(r):
        for h in range(c.H):
            lse[c.lse_at(b, h):c.lse_at(b, h) + c.nq_b(b)] = rb["lse"][h].float()
    return lse


def _flat(g, what):
    out = g.take(what)
    assert not bool(torch.isnan(out).any()), f"{what}: NaN (a guard was read)"
    return out


def _zeros_then_bound(got, ref, bound, what, rec, group):
    z = bound == 0
    assert bool((got[z] == 0).all()), (what, "not exactly 0 where the reference has no term:", int((got[z] != 0).sum()))
    _rec(rec, group, within(got, ref, bound, what))


def check_siblings(impl, c, rec=None):
    """pa_attention_probs (with and without head_mean), pa_attention_probs_grad (GRAD: torch.equal, integer products; CAM: zeros exact,
    the rest within EPS), pa_attention_rollout (ATTN and CAM, integer r_in, a = b_ = 0.5 and 1, one and two slices: EPS A)"""
    assert c.fam in ("select", "pair")
    i, r = attn_inputs(c), reference(c)
    conditions(c, i, r)
    lse = ref_lse(c, r)
    G_ = [rb["dP"] for rb in r]                                 # d_o v^T: integers
    for hm in (0, 1):
        off = map_offsets(c, hm)
        rc, g = impl.probs(c, i["qkv"], lse, hm)
        assert rc == PA_OK, (c.name, rc)
        got = _flat(g, c.name + " probs")
        rc, g = impl.probs(c, i["qkv"], lse, hm, d_o=i["d_o"], mode=PGRAD_CAM)
        assert rc == PA_OK, (c.name, rc)
        cam = _flat(g, c.name + " cam")
        for b, rb in enumerate(r):
            P, C = rb["P"], (rb["P"] * G_[b]).clamp_min(0)
            if hm:
                P, C = P.mean(0, keepdim=True), C.mean(0, keepdim=True)
            _zeros_then_bound(got[off[b]:off[b + 1]].view(P.shape), P, EPS * P, f"{c.name} probs hm{hm} seq {b}", rec, f"probs[dt{c.dt}]")
            _zeros_then_bound(cam[off[b]:off[b + 1]].view(C.shape), C, EPS * C, f"{c.name} cam hm{hm} seq {b}", rec, f"cam[dt{c.dt}]")
    off = map_offsets(c, 0)
    rc, g = impl.probs(c, i["qkv"], None, 0, d_o=i["d_o"], mode=PGRAD_GRAD)
    assert rc == PA_OK, (c.name, rc)
    got = _flat(g, c.name + " grad")
    for b in range(c.B):
        equal(got[off[b]:off[b + 1]].view(G_[b].shape), G_[b].float(), f"{c.name} probs_grad GRAD seq {b}")
    gen = torch.Generator().manual_seed(c.seed + 99)
    r_in = _ints(gen, -3, 3, NR * c.T)
    for mode in (ROLLOUT_ATTN, ROLLOUT_CAM):
        for ab in (0.5, 1.0):
            for slices in (1, 2):
                rc, g = impl.rollout(c, i["qkv"], lse, i["d_o"] if mode == ROLLOUT_CAM else None, r_in, mode, slices, ab, ab, G_SCALE)
                assert rc == PA_OK, (c.name, mode, ab, slices, rc)
                got = _flat(g, c.name + " rollout")
                for b, rb in enumerate(r):
                    N, nq = c.seq[b], c.nq_b(b)
                    M = rb["P"] if mode == ROLLOUT_ATTN else (rb["P"] * (G_SCALE * G_[b])).clamp_min(0)
                    M = M.mean(0)
                    rr = r_in[NR * c.cu[b]:NR * c.cu[b + 1]].view(NR, N).double()
                    ref = ab * rr + ab * (rr[:, :nq] @ M)
                    A = (ab * rr).abs() + ab * (rr[:, :nq].abs() @ M)
                    # a r_in is exact and carries no EPS; one f32 rounding of the sum on top
                    bound = EPS * ab * (rr[:, :nq].abs() @ M) + 2.0 ** -23 * A
                    _rec(rec, f"rollout[dt{c.dt}]", within(got[NR * c.cu[b]:NR * c.cu[b + 1]].view(NR, N), ref, bound,
                                                          f"{c.name} rollout mode {mode} a {ab} slices {slices} seq {b}"))


# ---- argument checks: leading dimensions below the row width (nothing is launched) ----------------------------------------
# (entry, argument made one 16-byte step too small)
LD_ARG_CASES = (("fwd", "ldqkv"), ("fwd", "ldo"), ("fwd_varlen", "ldqkv"), ("fwd_varlen", "ldo"), ("bwd", "ldqkv"), ("bwd", "ldo"),
                ("bwd", "lddqkv"), ("bwd_varlen", "ldqkv"), ("bwd_varlen", "ldo"), ("bwd_varlen", "lddqkv"), ("probs", "ldqkv"),
                ("probs_grad", "ldqkv"), ("probs_grad", "ldo"), ("rollout", "ldqkv"), ("rollout", "ldo"))
