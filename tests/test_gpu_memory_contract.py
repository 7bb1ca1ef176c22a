"""GPU: the memory contract of the C ABI (include/dau_conv.h), through the arena harness of abi_arena.py instead of
dau_conv._capi.Plan's shared grow-only workspace and torch's caching allocator, which hide three classes of kernel bug:

 1. a member's workspace requirement that is too small, or a store past the end of y / dx / a gradient: every buffer sits between
    1 MiB canary bands in ONE allocation, the workspace is exactly dau_conv_workspace_bytes long -- an overrun changes a canary;
 2. a read of scratch memory or of an output that the call itself has not written: workspace and outputs are poisoned (0x00, 0xFF =
    NaN, 0x7B = huge) and the results must not depend on the poison -- every border, padded tile, counter and partial sum must be
    written by a kernel of the same call, dau_conv_backward OVERWRITES, and the first offset-window pass must not accumulate;
 3. the "base not aligned" side of the staging kernels' vector / scalar switches: with skew 1 the activation buffers start one
    ELEMENT past a 256-byte boundary (as a contiguous slice x[1:] of a batch with odd S*H*W does), and the results must be the bits
    of the aligned call.

Every case runs forward + backward twice on one plan (the first round without an offset hint, the second with one) and checks both:
  a. canaries intact, inputs byte-identical, outputs that were not requested still at their fill, dau_conv_check_status OK with
     max|mu| equal to numpy's, bit for bit;
  b. every output at the project's existing bar for the member and storage type against oracle.dau_oracle on the values the kernels
     read (util.assert_parity defaults for fp32; rel 2e-2 / floor 4e-3 for bf16 storage, test_gpu_bf16.py; rel 2e-3 / floor 1e-3 for
     f16 storage, test_gpu_f16.py; rel 2e-2 / floor 1e-2 for the DAU_FLAG_DENSE_BF16 product forms, test_gpu_fuzz.py) -- on the
     edge channels only where the layer is wide, as test_gpu_split_gather_dot_ring.py does;
  c. every output finite everywhere (under the 0xFF fill that is "overwritten in full"), and bit-identical across the three fills;
  d. bit-identical across skew 0 / skew 1.
(c) and (d) compare every (skew, fill) variant of a case with the first variant of it that ran, round by round; for plans with one
bucket set the two rounds of one variant run the same kernels on the same memory pattern, and must agree too: that is the
run-to-run identity the cross-variant comparison relies on, asserted in every such case.

Nothing here is meant to fault: every call uses the library as its header allows."""
import numpy as np
import pytest

import abi_arena as aa
from oracle import dau_oracle as orc
from util import assert_parity, make_inputs

pytestmark = pytest.mark.gpu

PARAMS = aa.GRADS
I, UT, SD, FP = 1 << 0, 1 << 1, 1 << 2, 1 << 3              # USE_INTERPOLATION, UNIT_TESTING, SINGLE_DIM_KERNEL, FORBID_POSITIVE_DIM1
BF16, STATIC, DENSE_BF16, WGRAD_ALWAYS = 1 << 4, 1 << 5, 1 << 6, 1 << 8
SPLIT, NO_SPLIT, F16, OUTLIERS = 1 << 9, 1 << 10, 1 << 11, 1 << 12
IO_FLAG = {"f32": 0, "bf16": BF16, "f16": F16}
ALGO_DIRECT = 1


class Case(object):
    """One plan + one set of inputs.  flags: everything but the storage flag (added from io).  corner: offsets written onto the
    first two units (+-corner on both axes: the corners of the dense kernel / the offset window).  expect: {plan.info key: value or
    predicate}: the path this case is here for exists in its plan.  edge: compare with the oracle on the four first and last
    channels only (wide layers).  budget: DAU_WORKSPACE_BUDGET_GB at plan creation.  outliers: (pattern, seed) of
    test_gpu_dense_outliers._outliers, and the ring member must report that it ran."""

    def __init__(self, name, shape, flags, k=9, io="f32", m=3.0, corner=None, ignore=0, algo=0, expect=None, edge=False,
                 budget=None, outliers=None, seed=None):
        self.name, self.shape, self.flags, self.k, self.io, self.m, self.corner = name, shape, flags, k, io, m, corner
        self.ignore, self.algo, self.expect, self.edge, self.budget, self.outliers = ignore, algo, expect or {}, edge, budget, outliers
        self.seed = seed if seed is not None else 1 + sum(ord(c) for c in name)

    def oracle_kw(self):
        return dict(ignore=self.ignore, use_interpolation=bool(self.flags & I), single_dim_kernel=bool(self.flags & SD),
                    forbid_positive_dim1=bool(self.flags & FP))


def _edge(n):
    return sorted(set(range(min(4, n))) | set(range(max(0, n - 4), n)))


_DATA = {}        # case name -> (inputs, want): computed once, shared by the variants, never changed
_FIRST = {}       # (case name, round) -> ({output: bits}, variant) of the first variant that ran


def _data(case):
    if case.name in _DATA:
        return _DATA[case.name]
    N, S, F, G, H, W = case.shape
    x, dy, w, mu1, mu2 = make_inputs(case.seed, N, S, F, G, H, W, case.k, case.m, ignore=case.ignore)
    if case.corner is not None:
        c = np.float32(case.corner)
        mu1.flat[0] = c; mu2.flat[0] = -c; mu1.flat[1] = -c; mu2.flat[1] = c
    if case.outliers:
        from test_gpu_dense_outliers import _outliers
        _outliers(np.random.RandomState(case.outliers[1]), mu1, mu2, case.outliers[0])
    if case.flags & SD:
        mu2[:] = 0.0
    inputs = dict(x=x, dy=dy, w=w, mu1=mu1, mu2=mu2, sigma=np.full((1, S, G, F), 0.5, np.float32))
    # what the kernels read: the 16-bit storage of x and dy, widened
    xr, dyr = (aa.widen(aa.to_storage(a, case.io), case.io) for a in (x, dy))
    kw = case.oracle_kw()
    bkw = dict(kw, unit_testing=bool(case.flags & UT))
    if not case.edge:
        full = (Ellipsis,)
        want = {"y": (full, orc.forward(xr, w, mu1, mu2, 0.5, **kw))}
        want.update({n: (full, v) for n, v in orc.backward(xr, dyr, w, mu1, mu2, 0.5, **bkw).items()})
    else:        # an output channel's y and parameter gradients need that channel's units only; an input channel's dx likewise
        fs, ss = _edge(F), _edge(S)
        want = {"y": ((slice(None), fs), orc.forward(xr, w[..., fs], mu1[..., fs], mu2[..., fs], 0.5, **kw))}
        g = orc.backward(xr, dyr[:, fs], w[..., fs], mu1[..., fs], mu2[..., fs], 0.5, need=PARAMS, **bkw)
        want.update({n: ((Ellipsis, fs), g[n]) for n in PARAMS})
        want["dx"] = ((slice(None), ss), orc.backward(xr[:, ss], dyr, w[:, ss], mu1[:, ss], mu2[:, ss], 0.5, need=("dx",), **bkw)["dx"])
    _DATA[case.name] = (inputs, want)
    return _DATA[case.name]


def _plan(case, monkeypatch):
    from dau_conv import _capi
    N, S, F, G, H, W = case.shape
    if case.budget:
        monkeypatch.setenv("DAU_WORKSPACE_BUDGET_GB", case.budget)
    plan = _capi.Plan(N, S, F, G, H, W, max_kernel_size=case.k, number_units_ignore=case.ignore, flags=case.flags | IO_FLAG[case.io],
                      algo=case.algo, sigma_hint=0.5)
    if case.budget:
        monkeypatch.delenv("DAU_WORKSPACE_BUDGET_GB")
    for key, val in case.expect.items():
        got = plan.info[key]
        assert val(got) if callable(val) else got == val, "%s: plan.info[%r] = %r: the plan lacks the path this case tests" % (case.name, key, got)
    return plan


def _bars(case, plan):
    """(bar of y / dx, bar of the parameter gradients): the existing ones, see the module docstring"""
    io_bar = {"f32": {}, "bf16": dict(rel=2e-2, floor=4e-3), "f16": dict(rel=2e-3, floor=1e-3)}[case.io]
    param_bar = {}
    if plan.info["gather_dense_bf16"]:
        io_bar = dict(rel=2e-2, floor=1e-2)
        if plan.info["gather_dense_bf16"] == 2:
            param_bar = dict(rel=2e-2, floor=1e-2)
    return io_bar, param_bar


def _check_report(rep, inputs, tag):
    from dau_conv import _capi
    assert rep.rc == _capi.DAU_OK, "%s: rc %d: %s" % (tag, rep.rc, _capi.lib.dau_conv_last_error())
    assert rep.status_rc == _capi.DAU_OK, "%s: check_status %d" % (tag, rep.status_rc)
    want_mx = np.float32(max(np.abs(inputs["mu1"]).max(), np.abs(inputs["mu2"]).max()))
    assert rep.max_abs_mu == want_mx, "%s: max|mu| %r, numpy says %r" % (tag, rep.max_abs_mu, want_mx)
    rep.assert_clean(tag)
    for n, v in rep.values.items():
        bad = int((~np.isfinite(v)).sum())
        assert bad == 0, "%s: %s holds %d non-finite values of %d (first at flat index %d)" % (tag, n, bad, v.size, int(np.flatnonzero(~np.isfinite(v))[0]))


def _compare_with_first(key, bits, variant, tag):
    if key not in _FIRST:
        _FIRST[key] = (bits, variant)
        return
    ref, ref_variant = _FIRST[key]
    for n in sorted(bits):
        differ = int((bits[n] != ref[n]).sum())
        assert differ == 0, "%s: %s differs in %d of %d values from the call with (skew, fill) = %s" % (tag, n, differ, bits[n].size, ref_variant)


def _bits(*reports):
    out = {}
    for rep in reports:
        out.update({n: aa.as_bits(v) for n, v in rep.outputs.items()})
    return out


def _run_case(case, skew, fill, monkeypatch):
    from dau_conv import _capi
    inputs, want = _data(case)
    plan = _plan(case, monkeypatch)
    io_bar, param_bar = _bars(case, plan)
    rounds = []
    for rnd in range(2):
        tag = "%s skew %d fill 0x%02X round %d" % (case.name, skew, fill, rnd)
        f = aa.forward(_capi, plan, inputs, case.io, skew, fill, outlier_status=bool(case.outliers))
        _check_report(f, inputs, tag + " forward")
        b = aa.backward(_capi, plan, inputs, case.io, skew, fill, outlier_status=bool(case.outliers))
        _check_report(b, inputs, tag + " backward")
        if case.outliers:
            from test_gpu_dense_outliers import _count
            count = _count(inputs["mu1"], inputs["mu2"], case.ignore)
            assert f.outliers == (count, True) and b.outliers == (count, True), (tag, f.outliers, b.outliers, count)
        values = dict(f.values, **b.values)
        for n in ("y", "dx") + PARAMS:
            idx, ref = want[n]
            assert_parity(values[n][idx], ref, tag + " " + n, **(io_bar if n in ("y", "dx") else param_bar))
        bits = _bits(f, b)
        rounds.append(bits)
        _compare_with_first((case.name, rnd), bits, (skew, fill), tag)
    if plan.info["bucket_sets"] == 1:      # both rounds ran the same kernels: run-to-run identity
        for n in sorted(rounds[0]):
            differ = int((rounds[0][n] != rounds[1][n]).sum())
            assert differ == 0, "%s skew %d fill 0x%02X: %s is not run-to-run identical (%d of %d values)" % (case.name, skew, fill, n, differ, rounds[0][n].size)


RAGGED = (3, 5, 9, 3, 13, 21)          # odd W, odd H*W, odd S*H*W and F*H*W: skew and plane bases are odd
T98, T96, TWOBLK = (2, 7, 5, 2, 9, 8), (2, 7, 5, 2, 9, 6), (2, 33, 130, 2, 12, 12)
SDOT = (5, 20, 24, 3, 13, 22)
SPLIT_ALL = {"gather_dense_split": 0b11100}
EXACT = {"gather_dense_split": 0, "algo_forward": 2, "algo_backward": 2}


def _dense(name, shape, r, io="f32", flags=I | SPLIT, **kw):
    # a unit at exactly +-r (3.99 standing in for 4, the layer's clip), as test_split_gather_against_oracle
    return Case("%s-r%d%s" % (name, r, "" if io == "f32" else "-" + io), shape, flags, m=float(r), corner=min(float(r), 3.99), io=io,
                expect=SPLIT_ALL, seed=43 + r, **kw)


# each family's first case: crossed with skew {0, 1} x the three fills
CROSSED = [
    Case("exact-k9", RAGGED, I | NO_SPLIT, expect=EXACT),
    _dense("split-9x8", T98, 2), _dense("split-9x8", T98, 3), _dense("split-9x8", T98, 4),
    Case("ring-27x27", (2, 20, 40, 3, 27, 27), I | SPLIT | OUTLIERS, outliers=("both_axes", 1009), seed=9,
         expect={"gather_dense_split": 0b111100}),
    Case("splitdot-ragged", SDOT, I | SPLIT, corner=3.0, expect=SPLIT_ALL),
    Case("bf16dense-9x8", T98, I | DENSE_BF16, io="bf16", m=3.99, expect={"gather_dense_bf16": 1}),
    Case("bf16dense-wgrad-9x8", T98, I | DENSE_BF16 | WGRAD_ALWAYS, io="bf16", m=3.99, expect={"gather_dense_bf16": 2}),
]
# storage types: both skews (the 16-bit formats have alignment switches of their own), fill 0xFF
STORAGE = [c for io in ("bf16", "f16") for c in (
    Case("exact-k9-" + io, RAGGED, I | NO_SPLIT, io=io, expect=EXACT),
    _dense("split-9x8", T98, 3, io=io),
    Case("splitdot-ragged-" + io, SDOT, I | SPLIT, io=io, corner=3.0, expect=SPLIT_ALL),
)]
SLABBED = lambda N: {"batch_slab_gather": lambda v: v < N, "batch_slab_dot": lambda v: v <= N}
# the budget and shapes of test_batch_slabs_under_a_workspace_budget (test_gpu_baseline_configs.py) and of test_batch_slabs
# (test_gpu_dense_outliers.py), one channel / row / column changed so that S*H*W and F*H*W are odd: the slabs after the first begin at
# an odd element even at skew 0
SLABS = [c for io in ("f32", "f16") for c in (
    Case("slabs-k17-" + io, (12, 5, 11, 3, 39, 35), I | NO_SPLIT, k=17, m=7.5, io=io, budget="0.0005", expect=SLABBED(12)),
    Case("slabs-ring-" + io, (8, 21, 41, 3, 27, 27), I | SPLIT | OUTLIERS, io=io, budget="0.0005", outliers=("percent", 13), seed=12,
         expect=dict(SLABBED(8), gather_dense_split=0b111100)),
)]
# everything else: skew 1, fill 0xFF -- the most revealing single setting
REST = [
    Case("exact-k17", RAGGED, I | NO_SPLIT, k=17, m=7.5, expect=EXACT),
    Case("exact-k33", RAGGED, I | NO_SPLIT, k=33, m=15.5, expect=EXACT),
    # the shape of test_f16_window_pass_plan: the first window pass must store, the later ones accumulate onto it
    Case("exact-k65-windows-f16", (2, 2, 20, 9, 37, 100), I | NO_SPLIT, k=65, m=20.0, io="f16", seed=13,
         expect={"gather_windows": lambda v: v > 1}),
    Case("exact-k65-windows", (2, 2, 20, 9, 37, 100), I | NO_SPLIT, k=65, m=20.0, seed=13, expect={"gather_windows": lambda v: v > 1}),
    Case("exact-k17-static", RAGGED, I | NO_SPLIT | STATIC, k=17, m=3.0, expect={"bucket_sets": 1}),
    Case("direct-k9", RAGGED, I | NO_SPLIT, algo=ALGO_DIRECT, expect={"algo_forward": 1, "algo_backward": 1}),
] + [_dense(n, s, r) for n, s in (("split-9x6", T96), ("split-two-blocks", TWOBLK)) for r in (2, 3, 4)] + [
    # the one-strip and one-region-row geometries of test_gpu_split_gather_dot_ring.py
    Case("splitdot-one-strip", (8, 256, 256, 4, 40, 9), I | SPLIT, corner=3.0, edge=True, expect=SPLIT_ALL, seed=302),
    Case("splitdot-one-region-row", (16, 256, 256, 4, 3, 40), I | SPLIT, corner=3.0, edge=True, expect=SPLIT_ALL, seed=303),
    Case("bf16dense-9x6", T96, I | DENSE_BF16, io="bf16", m=3.0, expect={"gather_dense_bf16": 1}),
    Case("bf16dense-wgrad-9x6", T96, I | DENSE_BF16 | WGRAD_ALWAYS, io="bf16", m=3.0, expect={"gather_dense_bf16": 2}),
    # flag forms, once on the exact path and once on the dense path
    Case("exact-unit-testing", RAGGED, I | NO_SPLIT | UT, expect=EXACT),
    Case("exact-single-dim", RAGGED, I | NO_SPLIT | SD, expect=EXACT),
    Case("exact-forbid-positive", RAGGED, I | NO_SPLIT | FP, expect=EXACT),
    Case("exact-no-interpolation", RAGGED, NO_SPLIT, expect=EXACT),
    Case("exact-ignore1", RAGGED, I | NO_SPLIT, ignore=1, expect=EXACT),
    _dense("split-unit-testing", T98, 3, flags=I | SPLIT | UT),
    _dense("split-single-dim", T98, 3, flags=I | SPLIT | SD),
    _dense("split-forbid-positive", T98, 3, flags=I | SPLIT | FP),
    _dense("split-no-interpolation", T98, 3, flags=SPLIT),
    _dense("split-ignore1", T98, 3, ignore=1),
]

VARIANTS = ([(c, skew, fill) for c in CROSSED for skew in (0, 1) for fill in aa.FILLS]
            + [(c, skew, 0xFF) for c in STORAGE + SLABS for skew in (0, 1)]
            + [(c, 1, 0xFF) for c in REST])


def test_case_names_are_unique():
    names = [c.name for c in CROSSED + STORAGE + SLABS + REST]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("case, skew, fill", VARIANTS, ids=["%s-skew%d-fill%02X" % (c.name, s, f) for c, s, f in VARIANTS])
def test_memory_contract(case, skew, fill, monkeypatch):
    _run_case(case, skew, fill, monkeypatch)


# ---- need_mask, the two-step parameter gradients, a declared size one byte short: once on the exact and once on the dense path ----
KINDS = {"exact": Case("mask-exact", RAGGED, I | NO_SPLIT, expect=EXACT),
         "split": Case("mask-split", SDOT, I | SPLIT, corner=3.0, expect=SPLIT_ALL)}
_ALL = {}


def _need_all(kind, monkeypatch):
    """the NEED_ALL call of a kind (k = 9: one bucket set, no hint to speak of), once"""
    from dau_conv import _capi
    if kind not in _ALL:
        case = KINDS[kind]
        rep = aa.backward(_capi, _plan(case, monkeypatch), _data(case)[0], case.io, 1, 0xFF)
        _check_report(rep, _data(case)[0], case.name + " NEED_ALL")
        _ALL[kind] = _bits(rep)
    return _ALL[kind]


MASKS = {"dx": 1, "params": 2 | 4 | 8 | 16, "no-dsigma": 31 & ~16, "dmu1": 4}


@pytest.mark.parametrize("mask", sorted(MASKS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_need_mask(kind, mask, monkeypatch):
    """The gradients a mask requests are the bits of the NEED_ALL call; the others are passed as NULL, and their buffers in the arena
    (like y) keep their fill: nothing else was written."""
    from dau_conv import _capi
    case = KINDS[kind]
    inputs = _data(case)[0]
    ref = _need_all(kind, monkeypatch)
    rep = aa.backward(_capi, _plan(case, monkeypatch), inputs, case.io, 1, 0xFF, need_mask=MASKS[mask])
    _check_report(rep, inputs, "%s need_mask %s" % (case.name, mask))
    want = [n for n, b in (("dx", 1), ("dw", 2), ("dmu1", 4), ("dmu2", 8), ("dsigma", 16)) if MASKS[mask] & b]
    assert sorted(rep.outputs) == sorted(want) and sorted(rep.untouched) == sorted(set(aa.OUTPUTS) - set(want) - {"sums"})
    for n in want:
        assert np.array_equal(aa.as_bits(rep.outputs[n]), ref[n]), n


@pytest.mark.parametrize("fill", aa.FILLS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_param_sums_then_finalize(kind, fill, monkeypatch):
    """dau_conv_backward_param_sums into a poisoned sums buffer + dau_conv_finalize_param_grads == dau_conv_backward of the four kinds"""
    from dau_conv import _capi
    case = KINDS[kind]
    inputs = _data(case)[0]
    ref = _need_all(kind, monkeypatch)
    rep = aa.param_sums_finalize(_capi, _plan(case, monkeypatch), inputs, case.io, 1, fill)
    _check_report(rep, inputs, "%s sums + finalize" % case.name)
    assert sorted(rep.outputs) == sorted(PARAMS + ("sums",)) and sorted(rep.untouched) == ["dx", "y"]
    for n in PARAMS:
        assert np.array_equal(aa.as_bits(rep.outputs[n]), ref[n]), n
    assert np.array_equal(rep.outputs["sums"][0], rep.outputs["dw"][0])          # dw is the first kind's raw sum


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_declared_workspace_one_byte_short(kind, monkeypatch):
    """The same real buffer, declared one byte shorter than dau_conv_workspace_bytes: DAU_INVALID_ARGUMENT from all three entry points,
    and not a byte of the arena changes -- outputs and workspace (status block included: not even the memset was enqueued) keep their
    fill."""
    from dau_conv import _capi
    case = KINDS[kind]
    inputs = _data(case)[0]
    plan = _plan(case, monkeypatch)
    for call in (aa.forward, aa.backward, aa.param_sums_finalize):
        rep = call(_capi, plan, inputs, case.io, 0, 0x7B, declared_short=1)
        assert rep.rc == _capi.DAU_INVALID_ARGUMENT, (call.__name__, rep.rc)
        assert b"workspace too small" in _capi.lib.dau_conv_last_error()
        assert not rep.outputs and rep.untouched["workspace"] and rep.untouched["y"] and rep.untouched["dx"]
        rep.assert_clean("%s %s one byte short" % (case.name, call.__name__))
