"""The fp64 reference of decode_refs.py against independent compositions of existing pieces, the
conditions its bounds rest on for every case of the tables, and the proof that the GPU tests would
notice: a float32 emulation of the kernel's order of operations passes every case, and the same
emulation with one planted fault fails.  Runs without a GPU."""

import pytest
import torch

import neuronx_distributed_llama3_2_amd.ops as ops

import decode_refs as DR
import rowwise_refs as R
from decode_refs import BF16, F32, F64, GLU, PLAIN, RESID, ROPE_KV, Case

ALL = DR.all_cases()


def _fresh(c):
    return {k: t.clone() for k, t in DR.reference(c)[0].items()}


# ---- the float32 emulation -----------------------------------------------------------------------

def emulate(c, b, ks=1, fault=None):
    """dgemv in float32 in the kernel's order: per-chunk sum of squares, rows normalised and rounded
    to bf16, 8-element chunk products summed per k-slice and the slices in order, the epilogue's
    fp32 expressions and bf16 roundings; stores through the same views as the kernel.  `fault`
    plants one defect."""
    M, N, K, Nw = c.M, c.N, c.K, c.Nw
    v = DR.views(c, b)
    nch = K // 8
    X = DR.gathered_rows(c, v)
    if c.xcopy:
        v["xcopy"].copy_(X)
    if c.norm:
        f = X.float()
        chunks = (f * f).view(M, nch, 8).sum(-1)
        if fault == "ss_tail":
            chunks = chunks[:, :-1]
        rstd = torch.rsqrt(chunks.sum(-1) / K + torch.tensor(c.eps, dtype=F32))
        a = ((f * rstd[:, None]) * v["norm_w"].float()).to(BF16)
    else:
        a = X
    part = (a.float().view(M, 1, nch, 8) * v["w"].float().reshape(1, Nw, nch, 8)).sum(-1)     # [M, Nw, chunks]
    if fault == "drop_chunk":
        part[:, :, nch - 1] = 0
    if fault == "double_chunk":
        part[:, :, nch // 2] *= 2
    kc = ((K + ks - 1) // ks + 7) & ~7
    acc = torch.zeros(M, Nw, dtype=F32)
    for s in range(ks):
        kb = min(s * kc, K)
        ke = min(K, kb + kc)
        if kb < ke:
            acc = acc + part[:, :, kb // 8:ke // 8].sum(-1)
    y = v["y"]
    if c.epi == PLAIN:
        y.copy_(acc if c.yf else acc.to(BF16))
        if fault == "past_N":
            b["y"][0, N] = 1.0
    elif c.epi == RESID:
        yv = y.float()
        if c.yadd:
            yv = (yv + v["yadd"][:M].to(BF16).float()).to(BF16).float()
            v["yadd"][:M] = 0
            if fault == "yadd_left":
                v["yadd"][M - 1, N - 1] = 1.0
        y.copy_((yv + acc.to(BF16).float()).to(BF16))
    elif c.epi == GLU:
        g, u = acc[:, :N], acc[:, N:]
        y.copy_((g / (1 + torch.exp(-g)) * u).to(BF16))
    else:
        nq, nkv, D, half = c.nq, c.nkv, c.D, c.D // 2
        qk = (nq + nkv) * D
        xb = acc.to(BF16).float()
        heads = xb[:, :qk].reshape(M, nq + nkv, D)
        x1, x2 = heads[..., :half].clone(), heads[..., half:].clone()
        pt = v["pos"].clamp(0, c.P - 1)
        cs, sn = v["cos"][pt][:, None, :].repeat(1, nq + nkv, 1), v["sin"][pt][:, None, :].repeat(1, nq + nkv, 1)
        if fault == "cos_sin_swap":
            cs[0, nq, half - 1], sn[0, nq, half - 1] = sn[0, nq, half - 1].clone(), cs[0, nq, half - 1].clone()
        if fault == "partner_head":
            x2[:, nq] = heads[:, nq - 1, half:]
        rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1).to(BF16)
        out = torch.cat([rot.reshape(M, qk), xb[:, qk:].to(BF16)], 1)
        y.copy_(out)
        for m in range(M):
            ps = c.pos[m]
            if not 0 <= ps < c.Lmax:
                continue
            bq = m if fault == "cache_row_m" else m // c.T
            cb = c.cache_idx[bq] if c.cache_idx is not None and bq < len(c.cache_idx) else bq % c.B
            slot = ps + 1 if fault == "slot_off" else ps
            # through the whole buffer: a faulty slot or row may lie outside the view
            b["kc"][1 + cb, :nkv, 1 + slot, 4:4 + D] = rot[m, nq:]
            b["vc"][1 + cb, :nkv, 1 + slot, 4:4 + D] = out[m, qk:].reshape(nkv, D)


# ---- the reference against independent compositions ----------------------------------------------

def _close(a, b_, what, tol=1e-12):
    a, b_ = a.to(F64), b_.to(F64)
    err = (a - b_).abs() / (1.0 + b_.abs())
    assert float(err.max()) <= tol, f"{what}: {float(err.max())}"


COMPOSED = [Case(PLAIN, 3, 17, 520, True, "rand"), Case(PLAIN, 2, 17, 520, True, "rand", xadd=True),
            Case(RESID, 3, 17, 520, True, "rand", yadd=True), Case(GLU, 5, 12, 2056, True, "rand"),
            Case(GLU, 5, 12, 520, False, "int"),
            DR.rope_case(8, (4, 2, 64), 2, 520, True, "rand", shift=1),
            DR.rope_case(5, (3, 1, 8), 1, 40, True, "int", shift=0, xidx=True, xcopy=True),
            DR.rope_case(4, (2, 2, 72), 2, 40, False, "int", shift=3, use_idx=False)]


@pytest.mark.parametrize("c", COMPOSED, ids=lambda c: c.id)
def test_reference_matches_composition_of_existing_pieces(c):
    """rms_norm_reference (on doubles), a double matmul, rope_ref / swiglu_fwd_ref and a plain
    cache scatter give the reference's values."""
    b, outs, info = DR.reference(c)
    v = DR.views(c, b)
    M, N = c.M, c.N
    if c.xidx is not None:
        X = torch.nn.functional.embedding(v["xidx"].clamp(0, c.xrows - 1), v["x"].double())
        X[(v["xidx"] < 0) | (v["xidx"] >= c.xrows)] = 0
    else:
        X = v["x"].double()
    if c.xadd:
        X = (X.float() + v["xadd"][:M].to(BF16).float()).to(BF16).double()
    if c.xcopy:
        assert torch.equal(outs["xcopy"]["ref"][:M], X)
    a = ops.rms_norm_reference(X, v["norm_w"].double(), float(torch.tensor(c.eps, dtype=F32))) if c.norm else X
    _close(a, info["n64"] if c.norm else info["a"], "normalised rows", tol=2e-6)   # rms_norm_reference works in fp32
    acc = info["a"].double() @ v["w"].double().t()
    yref = outs["y"]["ref"][:M, :N]
    if c.epi == PLAIN:
        _close(yref, acc, "plain")
    elif c.epi == RESID:
        y1 = v["y"].double()
        if c.yadd:
            y1 = (v["y"].float() + v["yadd"][:M].to(BF16).float()).to(BF16).double()
            assert bool((outs["yadd"]["ref"][:M] == 0).all()) and bool(outs["yadd"]["written"][:M].all())
            assert not bool(outs["yadd"]["written"][M:].any())
        _close(yref, y1 + acc.float().to(BF16).double(), "resid")
    elif c.epi == GLU:
        _close(yref, R.swiglu_fwd_ref(acc), "glu")
    else:
        qk = (c.nq + c.nkv) * c.D
        xb = acc.float().to(BF16)
        pos = torch.tensor(c.pos).clamp(0, c.P - 1)
        rot, floor = R.rope_ref(xb, 0, c.nq + c.nkv, c.D, v["cos"], v["sin"], pos, 1.0)
        _close(yref[:, :qk], rot, "rope")
        assert bool((outs["y"]["floor"][:M, :qk] >= floor).all())
        kc = torch.full((c.B, c.nkv, c.Lmax, c.D), float("nan"), dtype=F64)
        vc = kc.clone()
        for m in range(M):
            if 0 <= c.pos[m] < c.Lmax:
                row = c.cache_idx[m // c.T] if c.cache_idx is not None else m // c.T
                kc[row, :, c.pos[m]] = rot[m, c.nq * c.D:].reshape(c.nkv, c.D)
                vc[row, :, c.pos[m]] = (xb if c.kind == "int" else acc)[m, qk:].double().reshape(c.nkv, c.D)
        for name, want in (("kc", kc), ("vc", vc)):
            ref = DR.out_views(c, {name: outs[name]["ref"]})[name]
            wr = DR.out_views(c, {name: outs[name]["written"]})[name]
            assert torch.equal(wr, ~torch.isnan(want)), name + ": the set of written slots"
            _close(ref[wr], want[wr], name)
            assert int(outs[name]["written"].sum()) == int(wr.sum()), name + ": nothing outside the view"


def test_tie_helpers():
    v = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 - 2.0 ** -9, 3.0 - 2.0 ** -7, 0.0, -(2.0 + 2.0 ** -7) * (1 + 2.0 ** -21)], dtype=F64)
    assert DR.bf16_ulp(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0 ** -6, 0.0, 2.0 ** -6]
    assert DR.tie_distance(v)[:4].tolist() == [2.0 ** -8, 0.0, 0.0, 0.0]
    assert DR.near_tie(v).tolist() == [False, True, True, True, False, True]


# ---- the conditions of the bounds, for every case ------------------------------------------------

def test_case_table_covers_the_issue():
    ids = [c.id for c in ALL]
    assert len(set(ids)) == len(ids)
    assert {c.M for c in ALL} == set(range(1, 9))
    assert {8, 40, 520, 2048, 2056, 4104, 8200} <= {c.K for c in ALL}
    assert {(c.nq, c.nkv, c.D) for c in ALL if c.epi == ROPE_KV} == set(DR.ROPE_HEADS)
    used = DR.wide_cases() + DR.split_cases() + DR.mfma_long_cases() + DR.other_cases(range(1, 9))
    used += [c for M in range(1, 9) for c in DR.default_cases(M)]
    used += [c for K in (8, 520, 4104) for c in DR.variants(GLU, 1, 5, K)] + DR.rope_cases((3, 1, 8), (1,))
    assert set(used) <= set(ALL), "every case the GPU tests run is walked here"
    for c in ALL:
        assert c.norm or c.kind == "int"
        if c.epi == ROPE_KV:
            assert c.P != c.Lmax and c.B > c.M // c.T and c.N == (c.nq + 2 * c.nkv) * c.D
            slots = [(cb, ps) for _, cb, ps in DR.cache_rows(c)]
            assert len(set(slots)) == len(slots), "two rows of a case must not share a cache slot"
    gates = torch.cat([DR.reference(c)[2]["g"].reshape(-1) for c in ALL if c.epi == GLU and c.kind == "int" and c.K >= 520])
    assert float(gates.min()) <= -16 and float(gates.max()) >= 16 and float(gates.abs().max()) <= 24
    pos_seen = {(p, c.Lmax, c.P) for c in ALL if c.epi == ROPE_KV for p in c.pos}
    for L, P in ((5, 9), (9, 5)):
        assert {(p, L, P) for p in (0, L - 1, L, -1, P - 1, P + 3)} <= pos_seen


def _live_rows(c, v, X):
    """Rows that are not the zero row of an id outside the table."""
    if c.xidx is None:
        return torch.ones(X.shape[0], dtype=torch.bool)
    return (v["xidx"] >= 0) & (v["xidx"] < c.xrows)


@pytest.mark.parametrize("part", range(8))
def test_every_case_meets_its_conditions_and_the_emulation_passes(part):
    for c in ALL[part::8]:
        b, outs, info = DR.reference(c)
        v = DR.views(c, b)
        if c.kind == "int":
            g = 2.0 ** min(min(DR.row_exponent(c, m) for m in range(c.M)), 0) if not c.norm else 1.0
            assert float(info["absacc"].max()) < 2.0 ** 24 * g, c.id
            assert bool((info["acc"] / g == torch.round(info["acc"] / g)).all()), c.id
            assert not bool(info["tie_a"].any())
            if c.norm:
                X = info["X"].double()
                live = _live_rows(c, v, X)
                r = torch.tensor([DR.row_exponent(c, m) for m in range(v["x"].shape[0])], dtype=F64)
                if c.xidx is not None:
                    r = r[v["xidx"].clamp(0, c.xrows - 1)]
                assert torch.equal(X.pow(2).mean(-1)[live], (4.0 ** r)[live]), c.id
                n64 = info["n64"][live]
                assert torch.equal(info["a"].double()[live].abs(), v["norm_w"].double().expand_as(info["n64"])[live]), c.id
                assert float((DR.tie_distance(n64) / n64.abs()).min()) >= 2.0 ** -9 * (1 - 2.0 ** -8), c.id
                assert float((n64.abs() / info["a"].double()[live].abs() - 1).abs().max()) < 2.0 ** -16, c.id
            if c.epi == GLU:
                assert float(info["g"].abs().max()) <= 24, c.id
                if c.N >= 5:
                    assert bool((info["g"] == 0).any()), c.id
            for o in outs.values():      # bit-equal everywhere but RoPE and GLU
                w = o["written"]
                if c.epi in (PLAIN, RESID):
                    assert bool(o["exact"][w].all()), c.id
        else:
            X = info["X"].double()
            live = _live_rows(c, v, X)
            energy = X.pow(2).view(X.shape[0], -1, 8).sum(-1)
            share = energy / energy.sum(-1, keepdim=True).clamp_min(1e-300)
            for k in DR.heavy_chunks(c.K):
                assert float(share[live][:, k // 8].min()) >= 0.10, f"{c.id}: chunk at k = {k}"
            if c.K >= 520 and not c.xadd:
                rms = energy.sqrt()
                light = torch.ones(c.K // 8, dtype=torch.bool)
                light[[k // 8 for k in DR.heavy_chunks(c.K)]] = False
                ratio = rms[live][:, light].max() / rms[live][:, light].min()
                assert float(ratio) >= 2.0 ** 4, c.id
            assert DR.near_share(c, info) <= DR.NEAR_SHARE, f"{c.id}: near-tie share {DR.near_share(c, info)}"
        for ks in (1, 2, 4):
            got = _fresh(c)
            emulate(c, got, ks)
            DR.check_outputs(c, got, f" ks={ks}")


# ---- planted faults ------------------------------------------------------------------------------

GEMV_FAULT_CASES = [Case(PLAIN, 3, 17, 520, False, "int"), Case(PLAIN, 1, 1, 4104, True, "rand"),
                    Case(RESID, 2, 17, 2056, True, "int"), Case(GLU, 5, 12, 520, True, "rand"),
                    Case(PLAIN, 2, 17, 520, True, "rand", yf=True),
                    DR.rope_case(2, (1, 1, 16), 1, 40, True, "int", shift=0)]
ROPE_FAULT_CASES = [DR.rope_case(4, (3, 1, 8), 2, 40, False, "int", shift=0),
                    DR.rope_case(8, (4, 2, 64), 2, 520, True, "rand", shift=3),
                    DR.rope_case(2, (2, 2, 72), 1, 40, True, "int", shift=0, use_idx=False)]


def _fails(c, fault, ks=2):
    got = _fresh(c)
    emulate(c, got, ks)
    DR.check_outputs(c, got)                       # the same emulation passes without the fault
    got = _fresh(c)
    emulate(c, got, ks, fault)
    with pytest.raises(AssertionError):
        DR.check_outputs(c, got)


@pytest.mark.parametrize("fault", ["drop_chunk", "double_chunk"])
@pytest.mark.parametrize("c", GEMV_FAULT_CASES, ids=lambda c: c.id)
def test_planted_k_chunk_fault_fails(c, fault):
    _fails(c, fault)


@pytest.mark.parametrize("fault", ["cos_sin_swap", "partner_head", "slot_off"])
@pytest.mark.parametrize("c", ROPE_FAULT_CASES, ids=lambda c: c.id)
def test_planted_rope_kv_fault_fails(c, fault):
    _fails(c, fault)


@pytest.mark.parametrize("c", [c for c in ROPE_FAULT_CASES if c.T == 2], ids=lambda c: c.id)
def test_planted_cache_row_m_instead_of_sequence_fails(c):
    _fails(c, "cache_row_m")


@pytest.mark.parametrize("c", [Case(RESID, 3, 17, 520, True, "rand", yadd=True), Case(RESID, 1, 1, 8, False, "int", yadd=True)],
                         ids=lambda c: c.id)
def test_planted_yadd_left_nonzero_fails(c):
    _fails(c, "yadd_left")


@pytest.mark.parametrize("c", [Case(PLAIN, 3, 17, 520, False, "int"), Case(PLAIN, 2, 17, 520, True, "rand", yf=True)],
                         ids=lambda c: c.id)
def test_planted_write_past_n_fails(c):
    _fails(c, "past_N")


@pytest.mark.parametrize("c", [Case(PLAIN, 1, 17, 4104, True, "rand"), Case(GLU, 5, 12, 520, True, "rand"),
                               DR.rope_case(2, (1, 1, 16), 1, 520, True, "rand", shift=0), Case(RESID, 2, 1, 8, True, "rand")],
                         ids=lambda c: c.id)
def test_planted_tail_chunk_missing_from_sum_of_squares_fails(c):
    _fails(c, "ss_tail")
