"""Per-element checks of the fused decode GEMV (_C.dgemv, csrc/decode_fused.hip) against the fp64
reference of decode_refs.py: every epilogue on the VALU and the MFMA body, at the shapes that reach
their guards (empty k-slices, tails, rows past M, inactive waves, the split over workgroups), with
every output inside a sentinel-filled buffer.  Integer cases are bit-equal, random cases are held
to the a-priori bounds derived in decode_refs.py.

Every test records its worst err / bound ratio per epilogue and output (record_property
"worst_<epilogue>_<output>"; 0 for outputs that are bit-equal throughout).
"""

import contextlib
import itertools

import pytest
import torch

from neuronx_distributed_llama3_2_amd.ops import _ext

import decode_refs as DR
from decode_refs import GLU, PLAIN, RESID, ROPE_KV

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(autouse=True)
def _native():
    assert _ext.ext_available(), "HIP extension must be built for GPU tests"
    yield


@pytest.fixture
def worst(record_property):
    seen = {}

    def note(c, ratios):
        for k, r in ratios.items():
            name = f"{DR.EPI_NAME[c.epi]}_{k}"
            seen[name] = max(seen.get(name, 0.0), float(r))

    yield note
    for k, v in seen.items():
        record_property("worst_" + k, round(v, 4))


@contextlib.contextmanager
def knobs(C, **kw):
    """Set decode knobs (k0=..., k7=...) and put every knob back to its documented default."""
    try:
        for name, value in kw.items():
            C.decode_set_knob(int(name[1:]), value)
        yield
    finally:
        for which, value in DR.KNOB_DEFAULTS.items():
            C.decode_set_knob(which, value)


class Run:
    """A case on the device: inputs uploaded once, outputs restored from the pristine copy before
    every call."""

    def __init__(self, C, c):
        self.C, self.c = C, c
        self.pristine = {k: t.to(DEV) for k, t in DR.reference(c)[0].items()}
        self.buf = dict(self.pristine)

    def call(self):
        for k in DR.OUT_KEYS:
            if k in self.pristine:
                self.buf[k] = self.pristine[k].clone()
        self.C.dgemv(*DR.call_args(self.c, DR.views(self.c, self.buf)))
        return {k: self.buf[k] for k in DR.OUT_KEYS if k in self.buf}

    def check(self, worst, what=""):
        got = self.call()
        worst(self.c, DR.check_outputs(self.c, got, what))
        return got


def _sweep(C, worst, cases, combos):
    """Every case under every knob combination (a dict of knobs() keywords)."""
    for c in cases:
        run = Run(C, c)
        for kw in combos:
            with knobs(C, **kw):
                run.check(worst, " " + " ".join(f"{k}={v}" for k, v in kw.items()))


def _product(**axes):
    names = list(axes)
    return [dict(zip(names, vals)) for vals in itertools.product(*axes.values())]


VALU_COMBOS = _product(k7=(0,), k1=(1, 2, 4), k6=(0, 1), k3=(0, 1))


# ---- VALU body -----------------------------------------------------------------------------------

@pytest.mark.parametrize("K", DR.VALU_K)
@pytest.mark.parametrize("epi", [PLAIN, RESID], ids=["plain", "resid"])
def test_valu_plain_resid(epi, K, worst):
    """M = 1, 2, 3, 5, 8 (MM = 1, 2, 4, 8 with rows past M), N = 1 and 17 (one wave of a workgroup,
    a partly filled last workgroup), 1 / 2 / 4 k-slices, FMA and dot2, early reads on and off.
    K = 8: all but the first slice empty; 520: a tail inside a 512-step; 2056: a second round;
    4104: a second prologue trip."""
    _sweep(_ext.ext(), worst, DR.valu_cases(epi, K), VALU_COMBOS)


@pytest.mark.parametrize("K", DR.VALU_K)
def test_valu_glu(K, worst):
    """N = 1, 5, 12 gate / up pairs at one and two pairs per wave (an odd N leaves half a wave)."""
    _sweep(_ext.ext(), worst, DR.valu_cases(GLU, K), [dict(kw, k0=p) for kw in VALU_COMBOS for p in (1, 2)])


def test_valu_two_rows_per_wave(worst):
    """N = 16385 >= 16384: two rows per wave, the last wave holds one."""
    _sweep(_ext.ext(), worst, DR.wide_cases(), _product(k7=(0,), k1=(1, 4), k6=(0, 1)))


@pytest.mark.parametrize("occ", [7, 8])
def test_valu_forced_occupancy(occ, worst):
    """M = 1 on the two-row kernels (GLU, ROPE_KV) built for 7 and 8 waves per SIMD."""
    cases = [c for K in (8, 520, 4104) for c in DR.variants(GLU, 1, 5, K)]
    cases += [c for c in DR.rope_cases((3, 1, 8), (1,)) + DR.rope_cases((2, 1, 128), (1,)) if c.xidx is None]
    _sweep(_ext.ext(), worst, cases, _product(k7=(0,), k5=(occ,), k1=(1, 2, 4), k6=(0, 1)))


# ---- MFMA body -----------------------------------------------------------------------------------

def _mfma_sweep(C, worst, cases):
    for c in cases:
        run = Run(C, c)
        with knobs(C, k7=2):
            run.check(worst, " k7=2")
        if c.M >= 4:
            with knobs(C, k7=4):
                run.check(worst, " k7=4")


@pytest.mark.parametrize("K", DR.MFMA_K)
@pytest.mark.parametrize("epi", [PLAIN, RESID, GLU], ids=["plain", "resid", "glu"])
def test_mfma(epi, K, worst):
    """M = 2, 4, 5, 8 (rows 0-3 and 4-7 sit in different lane groups), N = 1, 17, 40 (GLU 1, 5, 12):
    tiles with one column, a partly filled second and third tile.  K = 8 and 40: one k-step with a
    tail; 520: two slices; 4104: sixteen slices, the last one empty.  Knob 7 = 2 for all of them and
    the default 4 for M = 4..8."""
    _mfma_sweep(_ext.ext(), worst, DR.mfma_cases(epi, K))
    _sweep(_ext.ext(), worst, DR.mfma_cases(epi, K, (6, 7)), [dict(k7=4)])


def test_mfma_long_rows_without_prologue(worst):
    """K = 8200: sixteen slices of 544 with a tail in the last."""
    _mfma_sweep(_ext.ext(), worst, DR.mfma_long_cases())


def test_mfma_split_over_workgroups(worst):
    """Knob 8 = 1 at K = 2048 (two parts) and 8200 (eight parts, the last three empty), every
    epilogue.  Two calls back to back give the same bits: the parts are summed in a fixed order
    and the last part resets the ticket."""
    C = _ext.ext()
    for c in DR.split_cases():
        run = Run(C, c)
        with knobs(C, k7=2, k8=1):
            first = run.check(worst, " split, first call")
            second = run.check(worst, " split, second call")
        for k in first:
            DR.assert_bit_equal(DR.bits(first[k]), DR.bits(second[k]), f"{c.id} {k}: second call differs")


# ---- ROPE_KV on both bodies ----------------------------------------------------------------------

@pytest.mark.parametrize("heads", DR.ROPE_HEADS, ids=lambda h: "h%d.%d.%d" % h)
def test_rope_kv_valu(heads, worst):
    """Positions {0, Lmax - 1, Lmax, -1, P - 1, P + 3} with tables longer and shorter than the cache,
    T = 1 and 2, a cache with more rows than sequences, with and without a permuted cache_idx,
    with and without the prologue, and the embedding gather (ids -1 and `rows` give zero rows)."""
    combos = _product(k7=(0,), k1=(1, 2, 4), k6=(0, 1), k3=(0, 1))
    _sweep(_ext.ext(), worst, DR.rope_cases(heads, DR.VALU_M), combos)


@pytest.mark.parametrize("heads", [h for h in DR.ROPE_HEADS if h != (1, 1, 2)], ids=lambda h: "h%d.%d.%d" % h)
def test_rope_kv_mfma(heads, worst):
    """The same under knob 7 = 2.  D = 16, 64, 128 run on MFMA tiles of 8 rotary pairs; D = 8 and 72
    (D / 2 is no multiple of 8) must be sent to the VALU body, even at M = 8."""
    _mfma_sweep(_ext.ext(), worst, DR.rope_cases(heads, DR.MFMA_M))


# ---- side inputs and the shipped dispatch --------------------------------------------------------

@pytest.mark.parametrize("body", ["valu", "mfma"])
def test_side_inputs(body, worst):
    """xadd under the prologue (PLAIN, GLU, ROPE_KV, also with the gather), yadd with more rows than
    M (the rows past M stay), the fp32 y."""
    C = _ext.ext()
    if body == "valu":
        _sweep(C, worst, DR.other_cases(range(1, 9)), _product(k7=(0,), k1=(0, 4), k3=(0, 1)))
    else:
        _mfma_sweep(C, worst, DR.other_cases(range(2, 9)))


@pytest.mark.parametrize("M", range(1, 9))
def test_default_dispatch(M, worst):
    """Every knob at its default: what the models run."""
    _sweep(_ext.ext(), worst, DR.default_cases(M), [{}])


def test_binding_rejections():
    C = _ext.ext()

    def t(*shape, dtype=BF16):
        return torch.zeros(*shape, device=DEV, dtype=dtype)

    def call(epi, x, nw, w, y, **kw):
        C.dgemv(epi, x, nw, 1e-5, w, y, 0, 0, 0, None, None, None, 1, None, None, None, **kw)

    with pytest.raises(RuntimeError, match="1..8 rows"):
        call(PLAIN, t(9, 16), None, t(4, 16), t(9, 4))
    with pytest.raises(RuntimeError, match="K / strides"):
        call(PLAIN, t(1, 12), None, t(4, 12), t(1, 4))
    with pytest.raises(RuntimeError, match="M \\* K <= 32768"):
        call(PLAIN, t(8, 4104), t(4104), t(4, 4104), t(8, 4))
    with pytest.raises(RuntimeError, match="xidx needs"):
        C.dgemv(ROPE_KV, t(5, 16), None, 1e-5, t(6, 16), t(2, 6), 1, 1, 2, t(4, 1, dtype=F32), t(4, 1, dtype=F32),
                torch.zeros(2, device=DEV, dtype=torch.int64), 1, t(2, 1, 4, 2), t(2, 1, 4, 2), None,
                xidx=torch.zeros(2, device=DEV, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="yadd is the RESID"):
        call(PLAIN, t(1, 16), None, t(4, 16), t(1, 4), yadd=t(1, 4, dtype=F32))
