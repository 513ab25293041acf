"""fp64 references, per-element bounds and case tables of the flash-attention kernels
(csrc/flash_attn_fwd.hip, csrc/flash_attn_bwd.hip: plain, DROP and RANGE instantiations).

Plain module (like rowwise_refs.py / decode_refs.py), shared by test_attention_refs.py (CPU) and
test_flash_attention_gpu.py.  Every reference is written out from the definition in double on the
inputs' own device and returns, next to each output, the absolute `floor` of that output built
from the absolute values of the summands of each element's own expression.  An output passes when
|out - ref| <= BF16_REL |ref| + floor for every element (rowwise_refs.assert_elementwise).

Definition.  q [B,Sq,Hq,D], k / v [B,Sk,Hkv,D], G = Hq / Hkv, x = scale q.k.  Query i sees key j
iff lo <= j < hi (RANGE), j <= i + causal_offset (causal) and j < Sk.  P = softmax of x over the
visible keys, lse its log-sum-exp; a row without a visible key has o = 0, lse = -inf.  Dropout:
keep = ops.attention_dropout.dropout_keep_mask, l and lse use the undropped P, the P.V operand
is PD = P keep / (1 - p).  The backward is defined on GIVEN o (bf16) and lse (fp32):
P = exp(x - lse), delta = sum_d dO o, dP = dO V^T (times keep / (1 - p)), dS = P (dP - delta),
dQ = scale dS K, dK = scale sum_group dS^T Q, dV = sum_group PD^T dO.

Where the bounds come from (u = 2^-24; rules as at the top of rowwise_refs.py).  None of the
constants below is a measured number.

Forward, one row (n visible keys, nt = ceil(Sk / 64) key tiles, X = max visible |x|):
* s is a D-term fp32 accumulation of exact bf16 products: |ds| <= D u sum_d |q_d k_d|, carried
  into p through the exponential as the relative error scale * that.
* p = exp2(fma(s, c, -m)), c = fp32(scale) * fp32(log2 e): c is off by 2 u relative, which moves
  the argument by 2 u (|x| + |m|) <= 4 u X (natural-log units); the fma rounds once, u |arg| <=
  2 u X (m is a stale running max: at most the row's true max and at least the tile max - 8 log2
  units, so p <= 2^8, no overflow, and |arg| <= 2 X log2 e); v_exp_f32 adds 1 ulp = 2 u
  (rel_expf of rowwise_refs.py).  Together (6 X + 2) u.  m itself cancels in o and lse.
* every rescale multiplies l and the accumulators by alpha = exp2(m_old - m_new): argument
  rounding u |m_old - m_new| <= 2 u X, the instruction 2 u, the product u; at most one per tile:
  nt (2 X + 3) u.
  E_k = scale D u sum_d|q_d k_d| + (6 X + 2 + nt (2 X + 3)) u is the relative error of summand k.
* P is rounded to bf16 before P.V (after the fp32 product with 1 / (1 - p) under dropout, one
  more u): ub P_k |v_kd| absolute per summand, whatever the ties, with ub = 2^-8 = BF16_REL / 2 the
  unit roundoff of bf16 (8 significant bits: spacing 2^-7 in [1, 2), half of it relative to a value
  just above 1; rowwise_refs.py's "round-to-nearest to bf16 costs up to 2^-8 |ref|").  2^-9 is NOT
  a bound for it: 0.3310 rounds to 0.330078125, off by 1.43 * 2^-9 relative
  (test_attention_refs.py::test_bf16_unit_roundoff), and a row of three keys reaches it.
* P.V is an n-term fp32 accumulation: n u sum_k PD_k |v_kd|.
* l is an n-term fp32 sum of the unrounded p: relative error max_k E_k + n u; 1 / l and the
  product with it add 3 u.
  o floor_d = sum_k PD_k |v_kd| (ub + E_k + (n + 1) u) + (max E + (n + 3) u) sum_k PD_k |v_kd|.
* the final bf16 rounding of o: BF16_REL |ref| (2^-8 for the rounding, 2^-8 slack).
* lse = (m + log2 l) ln 2 stays fp32: the relative error of l passes through the logarithm as
  an absolute one, max E + n u; v_log_f32, the sum, the product with the rounded ln 2 and the
  2 u of c acting on m cost u-multiples of their operands:
  lse bound = max E + (n + 4) u + 4 u (X + |lse|)  -- u times the score range and the key count.

Census inputs (exact counts): q = 0, v[k, d] = [k % D == d].  Then s = 0, every p = 1 exactly
(bf16(1) = 1), l = the number of visible keys and the accumulators hold small integers: the only
roundings are 1 / l (1 ulp), the product and the final bf16 one.  o is held to BF16_REL |ref| with
no floor (under dropout the common factor bf16(1 / (1 - p)) is the same for every kept key; for the
p of the tables it is exact (p = 0.5) or off by 0.8 * 2^-9 relative (p = 0.1: 1.1111 -> 1.109375), within the 2^-8 slack
inside BF16_REL), lse = ln(count) to 8 u |lse| (v_log_f32 1 ulp, two
products).

Backward, element (i, j) of the P / dS tile:
* nlse = -lse / scale is rounded twice (1 / scale, the product) and is the initial value of the
  (D + 1)-term accumulation of s: |d(scale s - lse)| <= (D + 3) u (|lse| + scale sum_d|q_d k_d|);
  the product with c costs 3 u |x - lse|, v_exp_f32 2 u:
  EP = (D + 3) u (|lse| + scale sum_d|q_d k_d|) + (3 |x - lse| + 2) u, relative, on P.
* delta is a D-term fp32 sum: D u sum_d|dO_d o_d|; dP - delta is a (D + 1)-term accumulation
  started at -delta (under dropout: an fma of the accumulated dP with keep / (1 - p) and -delta):
  EdP = (D + 3) u (|delta| + ks sum_d|dO_d v_d|) + D u sum_d|dO_d o_d|, absolute.
* dS = P (dP - delta) is one fp32 product rounded to bf16 (ub):
  EdS = |dS| (ub + EP + 2 u) + P EdP, absolute.
* dQ = scale sum_j dS K: fp32 accumulation over the Sk keys in any order (MFMA chains, the D = 64
  key-half sum in LDS, atomics across key blocks): floor = scale sum_j (EdS + (Sk + 2) u |dS|) |k_jd|.
* dK = scale sum_{g, i} dS^T Q: n = G Sq leaf terms in any tree (query tiles, heads of the group,
  item slabs summed in item order): floor = scale sum (EdS + (n + 2) u |dS|) |q_id|.
* dV = sum_{g, i} bf16(P ks) dO: floor = sum PD (ub + EP + (n + 2) u) |dO_id|.
* final bf16 rounding of dq, dk, dv (after the fp32 product with scale): BF16_REL |ref|.
Census backward inputs make every summand non-negative (so the floor is about 2^-8 of the
value, the bound about 1.2 % of it); they use the same bounds.

Exact values: rows without a visible key give o = +0 and lse = -inf bit for bit; their dq rows,
and the dk / dv rows of keys no query sees, are +0 bit for bit (accumulators start at +0, and
+0 + -0 = +0).
"""

import math
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from neuronx_distributed_llama3_2_amd.ops.attention_dropout import dropout_keep_mask
from neuronx_distributed_llama3_2_amd.ops.attention_ranges import KeyRanges

from rowwise_refs import BF16_REL, TINY, U, assert_bit_equal, assert_elementwise, f64

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
P_RND = BF16_REL / 2       # ub: unit roundoff of bf16 (round to nearest, relative)
TILE_N = 64                # forward key tile
BLOCK_K = 256              # backward key block
BLOCK_Q = 32               # backward query tile
RESCALE_LOG2 = 8.0         # forward deferred-rescale threshold
MAX_KEYS = 704             # size cap of the case tables
SENS = 4.0                 # census sensitivity: a flipped pair moves an output by >= SENS * bound


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    kind: str                    # "fwd" | "bwd"
    D: int
    B: int
    Sq: int
    Sk: int
    Hq: int
    Hkv: int
    causal: bool = True
    off: Optional[int] = None    # None: Sk - Sq (bottom-right alignment)
    scale: Optional[float] = None
    ranges: Optional[Tuple] = None   # per batch row (cycled): ((q_end, lo, hi), ...) or ("window", w)
    drop: Optional[Tuple] = None     # (p, seed, head_offset)
    inputs: str = "rand"         # census | census_q | census_k | rand | spike_over | spike_under | big
    layout: str = "pad"          # pad | fused (q / k / v views of one [S, B, W] buffer; Sq == Sk)
    chunk: int = 0               # backward work-item chunk: 0 = automatic

    @property
    def variant(self):
        return "range" if self.ranges is not None else "drop" if self.drop is not None else "plain"

    @property
    def G(self):
        return self.Hq // self.Hkv

    @property
    def offset(self):
        return self.Sk - self.Sq if self.off is None else self.off

    @property
    def softmax_scale(self):
        return 1.0 / math.sqrt(self.D) if self.scale is None else self.scale

    @property
    def census(self):
        return self.inputs.startswith("census")

    @property
    def name(self):
        s = f"{self.kind}-{self.variant}-{self.inputs}-D{self.D}-b{self.B}q{self.Sq}k{self.Sk}h{self.Hq}/{self.Hkv}"
        s += ("-c" + ("" if self.off is None else str(self.off))) if self.causal else "-nc"
        if self.scale is not None:
            s += f"-s{self.scale:g}"
        if self.drop is not None:
            s += "-p{:g}s{}o{}".format(*self.drop)
        if self.layout != "pad":
            s += "-" + self.layout
        if self.chunk:
            s += f"-ch{self.chunk}"
        return s

    def __str__(self):
        return self.name


def case_ranges(c, device="cpu"):
    """(lo, hi) int32 [B, Sq] of a RANGE case, else None."""
    if c.ranges is None:
        return None
    lo = torch.zeros(c.B, c.Sq, dtype=torch.int32)
    hi = torch.zeros(c.B, c.Sq, dtype=torch.int32)
    for b in range(c.B):
        spec = c.ranges[b % len(c.ranges)]
        if spec[0] == "window":
            qk = torch.arange(c.Sq, dtype=torch.int32) + c.offset
            lo[b] = (qk - spec[1] + 1).clamp(0, c.Sk)
            hi[b] = (qk + 1).clamp(0, c.Sk)
            continue
        q0 = 0
        for q_end, l, h in spec:
            lo[b, q0:q_end] = l
            hi[b, q0:q_end] = h
            q0 = q_end
        assert q0 >= c.Sq, f"{c}: range pieces end at {q0}"
    return lo.clamp(0, c.Sk).to(device), hi.clamp(0, c.Sk).to(device)


def key_ranges(c, device="cpu"):
    lh = case_ranges(c, device)
    return None if lh is None else KeyRanges(lh[0], lh[1], c.Sk)


def visibility(c, device="cpu", bug=None):
    """bool [B, 1, Sq, Sk].  bug: a planted mask error of the kernel emulation."""
    qi = torch.arange(c.Sq, device=device)[None, :, None]
    ki = torch.arange(c.Sk, device=device)[None, None, :]
    vis = torch.ones(c.B, c.Sq, c.Sk, dtype=torch.bool, device=device)
    if c.causal:
        vis = vis & ((ki < qi + c.offset) if bug == "causal_ge" else (ki <= qi + c.offset))
    if c.ranges is not None:
        lo, hi = (t.long()[:, :, None] for t in case_ranges(c, device))
        vis = vis & (ki >= (lo + 1 if bug == "lo_off_by_one" else lo)) & ((ki <= hi) if bug == "hi_inclusive" else (ki < hi))
    return vis[:, None]


def keep_scale(c, device="cpu", head_offset=None):
    """float64 [B, Hq, Sq, Sk]: keep / (1 - p), or None without dropout."""
    if c.drop is None:
        return None
    p, seed, ho = c.drop
    keep = dropout_keep_mask(seed, c.B, c.Hq, torch.arange(c.Sq, device=device), c.Sk, p, ho if head_offset is None else head_offset)
    return keep.to(F64) / (1.0 - p)


def _bhsd(t, G=1):
    t = f64(t).permute(0, 2, 1, 3)
    return t if G == 1 else t.repeat_interleave(G, dim=1)


def _group_sum(t, G):
    B, Hq, S, D = t.shape
    return t.view(B, Hq // G, G, S, D).sum(2)


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------

def fwd_ref(q, k, v, scale, vis, ks=None):
    """o [B,Sq,Hq,D], lse [B,Hq,Sq] in double with o_floor and lse_bound (see the module docstring).
    vis: bool, broadcastable to [B,Hq,Sq,Sk]; ks: keep / (1 - p) [B,Hq,Sq,Sk] or None."""
    D, Sk, G = q.shape[-1], k.shape[1], q.shape[2] // k.shape[2]
    q64, k64, v64 = _bhsd(q), _bhsd(k, G), _bhsd(v, G)
    s = q64 @ k64.transpose(-1, -2)
    sabs = q64.abs() @ k64.abs().transpose(-1, -2)
    vis = vis.expand(s.shape)
    x = scale * s
    m = torch.where(vis, x, torch.full_like(x, -math.inf)).max(-1).values
    live = torch.isfinite(m)
    ms = torch.where(live, m, torch.zeros_like(m))
    e = torch.where(vis, torch.exp(torch.where(vis, x, ms[..., None]) - ms[..., None]), torch.zeros_like(x))
    l = e.sum(-1)
    lse = torch.where(live, ms + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, -math.inf))
    P = e / torch.where(live, l, torch.ones_like(l))[..., None]
    PD = P if ks is None else P * ks
    o = PD @ v64
    n = vis.sum(-1).to(F64)
    nt = math.ceil(Sk / TILE_N)
    X = torch.where(vis, x.abs(), torch.zeros_like(x)).max(-1).values
    E = scale * D * U * sabs + ((6 * X + 2 + nt * (2 * X + 3)) * U)[..., None]
    Emax = torch.where(vis, E, torch.zeros_like(E)).max(-1).values
    A = PD @ v64.abs()
    o_floor = (PD * (P_RND + E + (n[..., None] + 1) * U)) @ v64.abs() + (Emax + (n + 3) * U)[..., None] * A
    lse_fin = torch.where(live, lse, torch.zeros_like(lse))
    lse_bound = Emax + (n + 4) * U + 4 * U * (X + lse_fin.abs())
    return dict(o=o.permute(0, 2, 1, 3), lse=lse, o_floor=o_floor.permute(0, 2, 1, 3), lse_bound=lse_bound, P=P, live=live)


def bwd_ref(q, k, v, o, lse, do, scale, vis, ks=None):
    """dq [B,Sq,Hq,D], dk / dv [B,Sk,Hkv,D] in double from the GIVEN o and lse, with their floors."""
    D, Sq, Sk, G = q.shape[-1], q.shape[1], k.shape[1], q.shape[2] // k.shape[2]
    q64, k64, v64, o64, do64 = _bhsd(q), _bhsd(k, G), _bhsd(v, G), _bhsd(o), _bhsd(do)
    lse64 = f64(lse)
    live = torch.isfinite(lse64)
    lf = torch.where(live, lse64, torch.zeros_like(lse64))[..., None]
    s = q64 @ k64.transpose(-1, -2)
    sabs = q64.abs() @ k64.abs().transpose(-1, -2)
    on = vis.expand(s.shape) & live[..., None]
    x = scale * s
    arg = torch.where(on, x - lf, torch.zeros_like(x))
    P = torch.where(on, torch.exp(arg), torch.zeros_like(x))
    delta = (do64 * o64).sum(-1, keepdim=True)
    dabs = (do64 * o64).abs().sum(-1, keepdim=True)
    kk = 1.0 if ks is None else ks
    dpabs = (do64.abs() @ v64.abs().transpose(-1, -2)) * kk
    dpraw = do64 @ v64.transpose(-1, -2)
    dS = P * (dpraw * kk - delta)
    PD = P * kk
    dq = scale * (dS @ k64)
    dk = scale * _group_sum(dS.transpose(-1, -2) @ q64, G)
    dv = _group_sum(PD.transpose(-1, -2) @ do64, G)
    EP = (D + 3) * U * (lf.abs() + scale * sabs) + (3 * arg.abs() + 2) * U
    EdP = (D + 3) * U * (delta.abs() + dpabs) + D * U * dabs
    EdS = dS.abs() * (P_RND + EP + 2 * U) + P * EdP
    n = G * Sq
    dq_floor = scale * ((EdS + (Sk + 2) * U * dS.abs()) @ k64.abs())
    dk_floor = scale * _group_sum((EdS + (n + 2) * U * dS.abs()).transpose(-1, -2) @ q64.abs(), G)
    dv_floor = _group_sum((PD * (P_RND + EP + (n + 2) * U)).transpose(-1, -2) @ do64.abs(), G)
    pm = lambda t: t.permute(0, 2, 1, 3)
    return dict(dq=pm(dq), dk=pm(dk), dv=pm(dv), dq_floor=pm(dq_floor), dk_floor=pm(dk_floor), dv_floor=pm(dv_floor),
                P=P, PD=PD, dS=dS, dpraw=dpraw)


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------

def _gen(c, salt=0):
    return torch.Generator().manual_seed((zlib.crc32(c.name.encode()) + salt) & 0x7FFFFFFF)


def make_inputs(c):
    """CPU tensors: q, k, v (bf16) and, for backward cases, do (bf16), o (bf16), lse (fp32)."""
    g = _gen(c)
    D = c.D
    qs, ks_ = (c.B, c.Sq, c.Hq, D), (c.B, c.Sk, c.Hkv, D)
    rn = lambda shape: torch.randn(shape, generator=g, dtype=F32)
    ri = lambda shape, lo, hi: torch.randint(lo, hi, shape, generator=g).to(F32)
    onehot_q = (torch.arange(c.Sq)[:, None] % D == torch.arange(D)[None, :]).to(F32)[None, :, None, :].expand(qs)
    onehot_k = (torch.arange(c.Sk)[:, None] % D == torch.arange(D)[None, :]).to(F32)[None, :, None, :].expand(ks_)
    if c.inputs == "census":                       # forward: o = (visible keys = d mod D) / (visible keys)
        t = dict(q=torch.zeros(qs), k=ri(ks_, -3, 4), v=onehot_k.clone())
    elif c.inputs in ("census_q", "census_k"):     # backward, see census_backward_inputs
        t = dict(q=torch.zeros(qs), k=onehot_k.clone(), v=ri(ks_, 0, 2)) if c.inputs == "census_q" else \
            dict(q=onehot_q.clone(), k=torch.zeros(ks_), v=ri(ks_, 0, 2))
    else:
        t = dict(q=rn(qs), k=rn(ks_), v=rn(ks_))
        if c.inputs != "rand":
            # a shared component on d = 0: every query carries 4, the planted keys beta, so the
            # planted keys' scores are 4 beta scale above (below) the others' for every row
            nats = dict(spike_over=9.0, spike_under=5.0, big=60.0)[c.inputs]
            beta = float(torch.tensor(nats / (4.0 * c.softmax_scale)).to(BF16))
            if c.inputs != "big":
                t["q"] *= 0.25                     # ordinary scores within about +-1 of each other
            t["q"][..., 0] = 4.0
            t["k"][..., 0] = 0.0
            if c.inputs == "big":
                sign = torch.randint(0, 2, (c.B, c.Sk, c.Hkv), generator=g).to(F32) * 2 - 1
                t["k"][..., 0] = beta * sign
            else:
                for key in {c.Sk - 2, min(70, c.Sk - 1)}:
                    if key >= TILE_N:              # late: a running max exists when the spike arrives
                        t["k"][:, key, :, 0] = beta
    t = {n: x.to(BF16) for n, x in t.items()}
    if c.kind == "bwd":
        vis, ksc = visibility(c), keep_scale(c)
        if c.census:
            # dO one-hot by q % D scaled by the row's visible-key count (so P dO is about 1 for every
            # pair, whatever the row), o = -1 on that column: delta = -w, dS = P w (v + 1) >= 0
            cnt = vis.sum(-1).to(F32).clamp(min=1.0)[:, 0, :, None, None]          # [B, Sq, 1, 1]
            t["do"] = (onehot_q * cnt).to(BF16)
            t["o"] = (-onehot_q).to(BF16)
            t["lse"] = fwd_ref(t["q"], t["k"], t["v"], c.softmax_scale, vis, None)["lse"].to(F32)
        else:
            t["do"] = rn(qs).to(BF16)
            f = fwd_ref(t["q"], t["k"], t["v"], c.softmax_scale, vis, ksc)
            t["o"], t["lse"] = f["o"].to(BF16), f["lse"].to(F32)
    return t


def reference(c, t, device=None):
    """The case's fp64 reference from inputs t (on t's device unless `device` is given)."""
    device = t["q"].device if device is None else device
    t = {n: x.to(device) for n, x in t.items()}
    vis, ksc = visibility(c, device), keep_scale(c, device)
    if c.kind == "fwd":
        return fwd_ref(t["q"], t["k"], t["v"], c.softmax_scale, vis, ksc)
    r = bwd_ref(t["q"], t["k"], t["v"], t["o"], t["lse"], t["do"], c.softmax_scale, vis, ksc)
    r["q_dead"] = ~(vis.any(-1).expand(c.B, c.Hq, c.Sq) & torch.isfinite(t["lse"]))            # [B, Hq, Sq]
    seen = (vis.expand(c.B, c.Hq, c.Sq, c.Sk) & torch.isfinite(t["lse"])[..., None]).any(2)     # [B, Hq, Sk]
    r["k_dead"] = ~seen.view(c.B, c.Hkv, c.G, c.Sk).any(2)                                      # [B, Hkv, Sk]
    return r


def check_outputs(c, got, ref, what=""):
    """Every output of the case inside its bound; exact zeros / -inf bit for bit.  Returns
    {output: worst err / bound}."""
    what = f"{c}{what}"
    dev = ref["lse" if c.kind == "fwd" else "dq"].device
    out = {}
    if c.kind == "fwd":
        o, lse = got["o"].to(dev), got["lse"].to(dev)
        dead = ~ref["live"]                                                    # [B, Hq, Sq]
        if bool(dead.any()):
            assert_bit_equal(o.permute(0, 2, 1, 3)[dead], torch.zeros_like(o.permute(0, 2, 1, 3)[dead]), what + " o of empty rows")
            assert_bit_equal(lse[dead], torch.full_like(lse[dead], -math.inf), what + " lse of empty rows")
        live = ref["live"]
        o_floor = 0.0 if c.census else ref["o_floor"]
        out["o"] = assert_elementwise(o, ref["o"], BF16_REL, o_floor, what + " o")
        lse_ref = ref["lse"][live]
        lse_bound = 8 * U * lse_ref.abs() if c.census else ref["lse_bound"][live]
        out["lse"] = assert_elementwise(lse[live], lse_ref, 0.0, lse_bound, what + " lse")
        return out
    for n in ("dq", "dk", "dv"):
        g = got[n].to(dev)
        dead = (ref["q_dead"] if n == "dq" else ref["k_dead"]).permute(0, 2, 1)    # [B, S, H]
        if bool(dead.any()):
            assert_bit_equal(g[dead], torch.zeros_like(g[dead]), f"{what} {n} rows that see nothing")
        out[n] = assert_elementwise(g, ref[n], BF16_REL, ref[n + "_floor"], f"{what} {n}")
    return out


# ------------------------------------------------------------------------------------------------
# census sensitivity
# ------------------------------------------------------------------------------------------------

def boundary_pairs(c):
    """{boundary: bool [B, Hq, Sq, Sk]} with at most one pair per row set: the pairs next to each
    mask boundary, on either side (a visible one to hide, a hidden one to show)."""
    vis = visibility(c).expand(c.B, c.Hq, c.Sq, c.Sk)
    qi = torch.arange(c.Sq)[None, None, :]
    out = {}

    def at(name, key):                       # key: long [B, 1|Hq, Sq]; rows whose key is outside [0, Sk) are left out
        key = key.expand(c.B, c.Hq, c.Sq)
        ok = (key >= 0) & (key < c.Sk)
        m = torch.zeros_like(vis)
        m.scatter_(3, key.clamp(0, c.Sk - 1)[..., None], ok[..., None])
        out[name] = m

    if c.causal:
        d = (qi + c.offset).expand(c.B, 1, c.Sq)
        at("causal-in", d)
        at("causal-out", d + 1)
    if c.ranges is not None:
        lo, hi = (x.long()[:, None, :] for x in case_ranges(c))
        at("lo-in", lo)
        at("lo-out", lo - 1)
        at("hi-in", hi - 1)
        at("hi-out", hi)
    at("Sk-in", torch.full((c.B, 1, c.Sq), c.Sk - 1))
    if c.drop is not None:                   # the keep bit of the row's last visible key
        last = (vis * torch.arange(1, c.Sk + 1)).max(-1).values - 1
        at("keep", last)
    # a pair is only a boundary pair if flipping it is a one-pair change of the mask as a whole:
    # an "-in" pair must be visible now, an "-out" pair hidden now only by this boundary's own rule
    for name in list(out):
        if name.endswith("-in") or name == "keep":
            out[name] = out[name] & vis
        else:
            out[name] = out[name] & ~vis
    return out


def census_sensitivity(c, t=None):
    """For every boundary and row: the largest |change| / bound over the reference outputs when
    that row's boundary pair is flipped.  Returns {boundary: (min over rows, rows checked)}."""
    assert c.census
    t = make_inputs(c) if t is None else t
    vis = visibility(c).expand(c.B, c.Hq, c.Sq, c.Sk)
    ksc = keep_scale(c)
    res = {}
    if c.kind == "fwd":
        base = fwd_ref(t["q"], t["k"], t["v"], c.softmax_scale, vis, ksc)
        for name, m in boundary_pairs(c).items():
            rows = m.any(-1)
            if not bool(rows.any()):
                continue
            if name == "keep":
                f = fwd_ref(t["q"], t["k"], t["v"], c.softmax_scale, vis, torch.where(m, 1.0 / (1.0 - c.drop[0]) - ksc, ksc))
            else:
                f = fwd_ref(t["q"], t["k"], t["v"], c.softmax_scale, vis ^ m, ksc)
            both = base["live"] & f["live"]
            r_o = ((f["o"] - base["o"]).abs() / (BF16_REL * base["o"].abs() + TINY)).permute(0, 2, 1, 3).max(-1).values
            fl = torch.where(both, base["lse"], torch.zeros_like(base["lse"]))
            r_l = torch.where(both, (torch.where(both, f["lse"], fl) - fl).abs() / (8 * U * fl.abs() + TINY),
                              torch.full_like(fl, math.inf))   # a row that dies or comes alive: -inf <-> finite
            r = torch.maximum(torch.nan_to_num(r_o, nan=0.0, posinf=math.inf), r_l)
            res[name] = (float(r[rows].min()), int(rows.sum()))
        return res
    # backward: lse is given, so a flipped pair (i, j) changes dV[j] by PD_ij dO_i, dK[j] by
    # scale dS_ij q_i and dQ[i] by scale dS_ij k_j, exactly -- with P, dS taken as if visible
    on = torch.ones_like(vis)
    full = bwd_ref(t["q"], t["k"], t["v"], t["o"], t["lse"], t["do"], c.softmax_scale, on, ksc)
    base = bwd_ref(t["q"], t["k"], t["v"], t["o"], t["lse"], t["do"], c.softmax_scale, vis, ksc)
    G = c.G
    q64, k64, do64 = _bhsd(t["q"]), _bhsd(t["k"], G), _bhsd(t["do"])
    bound = {n: (BF16_REL * base[n].abs() + base[n + "_floor"] + TINY).permute(0, 2, 1, 3) for n in ("dq", "dk", "dv")}
    live = torch.isfinite(t["lse"])
    for name, m in boundary_pairs(c).items():
        m = m & live[..., None]
        idx = m.nonzero()                             # [n, 4]: b, h, i, j
        if idx.numel() == 0:
            continue
        b, h, i, j = idx.unbind(1)
        if name == "keep":                            # the keep bit flips: PD and the dP term of dS move by P / (1 - p) (x dP)
            PD = (full["P"][b, h, i, j] / (1.0 - c.drop[0]))[:, None]
            dS = PD * full["dpraw"][b, h, i, j][:, None]
        else:
            dS, PD = full["dS"][b, h, i, j][:, None], full["PD"][b, h, i, j][:, None]
        r_q = (c.softmax_scale * dS * k64[b, h, j]).abs() / bound["dq"][b, h, i]
        r_k = (c.softmax_scale * dS * q64[b, h, i]).abs() / bound["dk"][b, h // G, j]
        r_v = (PD * do64[b, h, i]).abs() / bound["dv"][b, h // G, j]
        r = torch.cat([r_q, r_k, r_v], dim=1).max(-1).values
        res[name] = (float(r.min()), int(idx.shape[0]))
    return res


# ------------------------------------------------------------------------------------------------
# case tables
# ------------------------------------------------------------------------------------------------

DS = (64, 128)
HEADS = ((2, 2), (4, 1), (8, 1))           # Hq / Hkv = 1, 4, 8
FWD_SQ = (1, 31, 32, 33, 127, 128, 129, 257)
FWD_SK = (1, 63, 64, 65, 129, 193)
W8 = dict(B=8, Sq=65, Sk=65, Hq=64, Hkv=8)  # ceil(65 / 256) * 8 * 64 = 512 blocks: the 8-wave kernel at its smallest grid
W4 = dict(W8, B=7)                          # 448 blocks: the same problem on the 4-wave kernel


def forward_cases():
    out = []
    for D in DS:
        # every Sq with two Sk (one tile, a tile tail, odd and even tile counts), every group size
        for i, Sq in enumerate(FWD_SQ):
            for n, Sk in enumerate((FWD_SK[i % 6], FWD_SK[(i + 3) % 6])):
                Hq, Hkv = HEADS[(i + n) % 3]
                sh = dict(D=D, B=2 - (i + n) % 2, Sq=Sq, Sk=Sk, Hq=Hq, Hkv=Hkv)
                out.append(Case("fwd", inputs="census", **sh))                       # causal, default offset
                out.append(Case("fwd", inputs="rand", causal=False, scale=(0.3 if n else None), **sh))
                if Sq > Sk:                                                          # leading rows see nothing
                    out.append(Case("fwd", inputs="rand", **sh))
        # explicit offsets: negative, inside, >= Sk
        for off in (-40, -1, 0, 5, 129, 200):
            out.append(Case("fwd", D=D, B=1, Sq=129, Sk=129, Hq=4, Hkv=1, off=off, inputs="census"))
        out.append(Case("fwd", D=D, B=1, Sq=129, Sk=129, Hq=2, Hkv=2, off=-40, inputs="rand"))
        out.append(Case("fwd", D=D, B=2, Sq=257, Sk=257, Hq=4, Hkv=1, inputs="census", layout="fused"))
        out.append(Case("fwd", D=D, B=2, Sq=193, Sk=193, Hq=4, Hkv=2, inputs="rand", layout="fused", scale=0.2))
        out.append(Case("fwd", D=D, B=1, Sq=200, Sk=700, Hq=2, Hkv=1, inputs="rand"))
        # the rescale paths and large scores
        for inp in ("spike_over", "spike_under", "big"):
            out.append(Case("fwd", D=D, B=1, Sq=129, Sk=193, Hq=2, Hkv=1, causal=False, inputs=inp))
            out.append(Case("fwd", D=D, B=1, Sq=193, Sk=193, Hq=2, Hkv=1, inputs=inp))
        # 8-wave kernel at its smallest grid, and the same problem on the 4-wave kernel
        for sh in (W8, W4):
            out.append(Case("fwd", D=D, inputs="census", **sh))
            out.append(Case("fwd", D=D, inputs="rand", causal=False, **sh))
    return out


# rows 0-2 empty at the start of a wave, 14-17 in its middle, 30-31 at its end; single-key rows;
# lo / hi at 63, 64, 65; wave 1 (rows 32-63) is empty at a tile edge and skips every tile while its
# neighbours do not
R_SMALL = ((3, 0, 0), (8, 0, 1), (14, 0, 63), (18, 63, 63), (24, 63, 64), (30, 63, 65), (32, 65, 65),
           (64, 128, 128), (80, 128, 129), (100, 128, 193), (128, 129, 193), (140, 129, 193), (300, 192, 193))
# lo / hi at 255, 256, 257; the second workgroup starts at tile 3 (odd), the third at tile 4
R_LARGE = ((20, 0, 255), (40, 1, 256), (60, 2, 257), (100, 64, 257), (128, 200, 300), (160, 255, 300),
           (200, 255, 321), (256, 256, 321), (300, 257, 321))
R_DOCS = ((63, 0, 700), (64, 63, 700), (65, 64, 700), (129, 65, 700), (300, 129, 700))   # packed documents, with causal


def range_cases():
    out = []
    for D in DS:
        for inp in ("census", "rand"):
            out.append(Case("fwd", D=D, B=2, Sq=193, Sk=193, Hq=4, Hkv=2, causal=False, ranges=(R_SMALL, R_DOCS), inputs=inp))
            out.append(Case("fwd", D=D, B=2, Sq=289, Sk=321, Hq=2, Hkv=1, causal=False, ranges=(R_LARGE, R_SMALL), inputs=inp))
            out.append(Case("fwd", D=D, B=2, Sq=257, Sk=257, Hq=4, Hkv=1, ranges=(R_DOCS, ("window", 65)), inputs=inp,
                            layout="fused"))
            out.append(Case("fwd", D=D, B=1, Sq=100, Sk=321, Hq=2, Hkv=2, ranges=(R_LARGE,), inputs=inp))        # cross lengths
            out.append(Case("fwd", D=D, B=2, Sq=193, Sk=129, Hq=2, Hkv=1, ranges=(("window", 64), R_SMALL), off=-10,
                            inputs=inp))
        out.append(Case("fwd", D=D, inputs="census", ranges=(("window", 33), ((40, 0, 1), (70, 1, 65))), **W8))
        out.append(Case("fwd", D=D, inputs="census", ranges=(("window", 33), ((40, 0, 1), (70, 1, 65))), **W4))
    return out


SEEDS = (1234, 987654321)


def dropout_cases():
    out = []
    for D in DS:
        for i, (p, seed, ho) in enumerate(((0.1, SEEDS[0], 0), (0.5, SEEDS[1], 4), (0.5, SEEDS[0], 0), (0.1, SEEDS[1], 4))):
            inp = "census" if i % 2 == 0 else "rand"
            out.append(Case("fwd", D=D, B=2, Sq=65, Sk=193, Hq=4, Hkv=1, drop=(p, seed, ho), inputs=inp))      # causal, Sk > Sq
            out.append(Case("fwd", D=D, B=1, Sq=129, Sk=129, Hq=2, Hkv=2, causal=False, drop=(p, seed, ho),
                            inputs=("rand" if inp == "census" else "census")))
        out.append(Case("fwd", D=D, drop=(0.5, SEEDS[0], 4), inputs="census", **W8))
        out.append(Case("fwd", D=D, drop=(0.1, SEEDS[1], 0), inputs="rand", **W8))
        out.append(Case("fwd", D=D, drop=(0.5, SEEDS[0], 4), inputs="census", **W4))
    return out


BWD_SK = (1, 255, 256, 257, 513)
BWD_SQ = (1, 31, 32, 33, 257)
ONE_ITEM = 100000                      # a chunk above every block's iteration count
# keys >= 300 are past every query's range; the key block 256.. is seen by the queries 200.. only, so
# with chunk 8 its restricted tile space (2 tiles per head) leaves items without tiles; block 512 by none
R_BWD = ((100, 0, 100), (150, 100, 100), (200, 100, 256), (240, 255, 257), (300, 256, 300))
R_BWD2 = ((5, 0, 0), (31, 0, 1), (33, 1, 255), (300, 255, 256))


def backward_cases():
    out = []
    for D in DS:
        for i, Sk in enumerate(BWD_SK):
            for n, Sq in enumerate((BWD_SQ[i], BWD_SQ[(i + 2) % 5])):
                G = 4 if (i + n) % 2 else 1
                sh = dict(D=D, B=2 - (i + n) % 2, Sq=Sq, Sk=Sk, Hq=G * (2 if G == 1 else 1), Hkv=(2 if G == 1 else 1))
                chunk = (8, 0, ONE_ITEM)[(i + n) % 3]
                out.append(Case("bwd", inputs="census_q", chunk=chunk, **sh))
                out.append(Case("bwd", inputs="census_k", causal=False, chunk=chunk, **sh))
                out.append(Case("bwd", inputs="rand", causal=bool(n), scale=(None if n else 0.3), chunk=chunk, **sh))
        big = dict(D=D, B=1, Sq=257, Sk=513, Hq=4, Hkv=1)
        for chunk in (8, 0, ONE_ITEM):
            out.append(Case("bwd", inputs="census_q", chunk=chunk, **big))
            out.append(Case("bwd", inputs="census_k", chunk=chunk, **big))
            out.append(Case("bwd", inputs="rand", chunk=chunk, **big))
        out.append(Case("bwd", inputs="big", chunk=8, **big))
        out.append(Case("bwd", inputs="rand", layout="fused", D=D, B=2, Sq=257, Sk=257, Hq=4, Hkv=1, chunk=8))
        # whole key blocks with zero iterations (keys 256.. at offset 0), exact-zero dk / dv rows
        for inp in ("census_q", "census_k", "rand"):
            out.append(Case("bwd", D=D, B=1, Sq=100, Sk=600, Hq=4, Hkv=1, off=0, inputs=inp, chunk=8))
        out.append(Case("bwd", D=D, B=1, Sq=257, Sk=257, Hq=2, Hkv=2, off=-100, inputs="rand"))   # empty leading query rows
        # ranges: items without tiles, keys past every range, empty query rows
        for inp in ("census_q", "census_k", "rand"):
            out.append(Case("bwd", ranges=(R_BWD,), causal=False, inputs=inp, chunk=8, **big))
            out.append(Case("bwd", D=D, B=2, Sq=257, Sk=513, Hq=4, Hkv=1, ranges=(R_BWD2, ("window", 65)), inputs=inp))
            out.append(Case("bwd", D=D, B=2, Sq=33, Sk=257, Hq=2, Hkv=2, ranges=(R_BWD2, R_BWD), causal=False, inputs=inp,
                            chunk=ONE_ITEM))
        # dropout backward, the forward's masks
        for p, seed, ho in ((0.1, SEEDS[0], 0), (0.5, SEEDS[1], 4)):
            for inp in ("census_q", "census_k", "rand"):
                out.append(Case("bwd", D=D, B=2, Sq=65, Sk=257, Hq=4, Hkv=1, drop=(p, seed, ho), inputs=inp, chunk=8))
            out.append(Case("bwd", D=D, B=1, Sq=257, Sk=129, Hq=2, Hkv=2, drop=(p, seed, ho), inputs="rand", causal=False))
    return out


def all_cases():
    return forward_cases() + range_cases() + dropout_cases() + backward_cases()


def group(cases, size):
    """Chunks of a case list (one GPU test per chunk keeps every test within a few seconds)."""
    return [cases[i:i + size] for i in range(0, len(cases), size)]


# ------------------------------------------------------------------------------------------------
# sentinel layouts (used on whatever device the inputs are put on)
# ------------------------------------------------------------------------------------------------

def nan_like(shape, dtype, device):
    """A buffer filled with a quiet-NaN bit pattern (bf16 0x7FC1 / fp32 0x7FC00001: not the default NaN)."""
    if dtype == BF16:
        return torch.full(shape, 0x7FC1, dtype=torch.int16, device=device).view(BF16)
    return torch.full(shape, 0x7FC00001, dtype=torch.int32, device=device).view(F32)


class Slot:
    """A logical [B, S, H, D] tensor as a strided view inside a NaN-filled buffer.
    pad:  buffer [B, S + 2, H + 1, D + 8], view [:, 1:S+1, :H, 8:] -- NaNs before and after every row;
    sbhd: buffer [S + 2, B, H + 1, D + 8] viewed [B, S, H, D] -- non-contiguous leading dims;
    a fused slot is cut from a shared [S + 2, B, W] buffer by `fused_slots`."""

    def __init__(self, buf, view_fn):
        self.buf, self.view_fn = buf, view_fn
        self.view = view_fn(buf)

    @classmethod
    def make(cls, shape, device, kind="pad", dtype=BF16):
        B, S, H, D = shape
        if kind == "pad":
            return cls(nan_like((B, S + 2, H + 1, D + 8), dtype, device), lambda b: b[:, 1:S + 1, :H, 8:])
        return cls(nan_like((S + 2, B, H + 1, D + 8), dtype, device), lambda b: b[1:S + 1, :, :H, 8:].permute(1, 0, 2, 3))

    def fill(self, t):
        self.view.copy_(t)
        return self

    def snapshot(self):
        self.pristine = self.buf.clone()

    def assert_outside_untouched(self, what):
        inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=self.buf.device)
        self.view_fn(inside).fill_(True)
        bits = torch.int16 if self.buf.dtype == BF16 else torch.int32
        assert_bit_equal(self.buf.view(bits)[~inside], self.pristine.view(bits)[~inside], what + ": bytes outside the output view")


def fused_slots(S, B, heads, D, device):
    """Views [B, S, h, D] for every h in `heads`, laid side by side in one NaN-filled [S + 2, B, W]
    buffer (rows 0 and S + 1 stay NaN): the layout rope_attention gives the kernels."""
    W = sum(heads) * D
    buf = nan_like((S + 2, B, W), BF16, device)
    slots, col = [], 0
    for h in heads:
        fn = (lambda c0, hh: lambda b: b[1:S + 1, :, c0:c0 + hh * D].unflatten(-1, (hh, D)).permute(1, 0, 2, 3))(col, h)
        slots.append(Slot(buf, fn))
        col += h * D
    return slots


def flat_slot(shape, device):
    """A contiguous fp32 [..] view at offset 16 of a NaN-filled flat buffer (lse must be contiguous)."""
    n = math.prod(shape)
    return Slot(nan_like((n + 48,), F32, device), lambda b: b[16:16 + n].view(shape))
