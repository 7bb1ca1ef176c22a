"""GPU: the chunk-pair tap loop of the two-limb f16 gather-sum (k_dense_split.hip: one v_mfma_f32_16x16x32_f16 covers a tap of
TWO 16-channel chunks; radii that did not switch run the same cases through their 32x32x16 loop).  Shapes are the smallest that
reach each path of the pairing: an even and an odd number of chunks in the forward pass and -- where the output channels play the
input's part -- in the dx pass, a ragged single chunk, dead waves beyond Cout, row and column tails, blocks of four and three
tiles, tall tiles and the block of four rows.  Bar: the fp32 one of tests/test_gpu_dense_split.py (1e-4 relative + 1e-6 of the
max-norm against the oracle).  A last chunk without a partner must add exact zeros, read nothing of an absent chunk (poisoned
workspace) and must not widen the reach of a non-finite input (compared with the 32x32x16 build of the same sources)."""
import numpy as np
import pytest
import torch

import abi_arena as aa
from oracle import dau_oracle as orc
from util import assert_parity, make_inputs, run_plan, tuning_capi, variant_capi

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _flags(capi, extra=0):
    return capi.FLAG_USE_INTERPOLATION | capi.FLAG_DENSE_SPLIT_F16 | extra


def _inputs(radius, N, S, F, G, H, W):
    r = float(radius)
    x, dy, w, mu1, mu2 = make_inputs(71 + radius, N, S, F, G, H, W, 9, r)
    c = min(r, 3.99)          # one unit at each corner of the radius (radius 4: the layer's clip)
    mu1.flat[0] = c; mu2.flat[0] = -c; mu1.flat[1] = -c; mu2.flat[1] = c
    return x, dy, w, mu1, mu2


def _oracle(key, x, dy, w, mu1, mu2):
    """the oracle's y and dx of a case, computed once and shared"""
    if key not in _ORACLE:
        want = orc.backward(x, dy, w, mu1, mu2, 0.5)
        _ORACLE[key] = dict(y=orc.forward(x, w, mu1, mu2, 0.5), dx=want["dx"], dw=want["dw"], dmu1=want["dmu1"], dmu2=want["dmu2"],
                            dsigma=want["dsigma"])
    return _ORACLE[key]


SHAPES = {
    "S16-F40": dict(N=2, S=16, F=40, G=2, H=9, W=27),        # one chunk forward; three chunks in dx, odd; row and column tails
    "S40-F32": dict(N=2, S=40, F=32, G=2, H=12, W=56),       # 3 / 2 chunks; blocks of 4 and 3 tiles; 8 + 4 rows
    "S7-F5": dict(N=2, S=7, F=5, G=2, H=9, W=27),            # ragged single chunk both ways
    "S64-F130": dict(N=1, S=64, F=130, G=2, H=12, W=20),     # 4 / 9 chunks; two channel blocks, dead waves beyond Cout
}


@pytest.mark.parametrize("radius", [2, 3, 4])
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_chunk_pairs_against_oracle(name, radius):
    from dau_conv import _capi
    s = SHAPES[name]
    N, S, F, G, H, W = (s[q] for q in ("N", "S", "F", "G", "H", "W"))
    x, dy, w, mu1, mu2 = _inputs(radius, N, S, F, G, H, W)
    plan = _capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5, flags=_flags(_capi))
    assert plan.info["gather_dense_split"] == 0b11100
    got = run_plan(plan, x, dy, w, mu1, mu2)
    want = _oracle((name, radius), x, dy, w, mu1, mu2)
    for key in ("y", "dx", "dw", "dmu1", "dmu2", "dsigma"):
        assert_parity(got[key], want[key], "pairs/r%d/%s/%s" % (radius, name, key))


@pytest.mark.parametrize("radius", [2, 3, 4])
@pytest.mark.parametrize("knobs", [dict(DAU_SPLIT_TALL="2", DAU_SPLIT_ROWS4="2"), dict(DAU_SPLIT_TALL="0", DAU_SPLIT_ROWS4="2")],
                         ids=["tall+rows4", "rows4"])
def test_forced_tall_tiles_and_block_of_four_rows(knobs, radius, monkeypatch):
    """28 x 28 with 40 -> 24 channels (3 / 2 chunks): seven tall tiles over 24 rows and the block of four rows, forced by the tuning
    build's knobs; the same sums as the production geometry of the same call, bit for bit (every form shares one tap loop)."""
    capi = tuning_capi()
    N, S, F, G, H, W = 1, 40, 24, 2, 28, 28
    x, dy, w, mu1, mu2 = _inputs(radius, N, S, F, G, H, W)
    plain = run_plan(capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5, flags=_flags(capi)), x, dy, w, mu1, mu2)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    got = run_plan(capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5, flags=_flags(capi)), x, dy, w, mu1, mu2)
    want = _oracle(("28x28", radius), x, dy, w, mu1, mu2)
    for key in ("y", "dx"):
        assert_parity(got[key], want[key], "pairs-forced/r%d/%s" % (radius, key))
        assert np.array_equal(got[key].view(np.uint32), plain[key].view(np.uint32)), key


@pytest.mark.parametrize("io", ["f16", "bf16"])
def test_sixteen_bit_activations(io):
    """S = 40 -> F = 24 (3 / 2 chunks) with binary16 / bfloat16 x, y, dy, dx: the storage bars of those formats for y and dx."""
    from dau_conv import _capi
    N, S, F, G, H, W = 2, 40, 24, 2, 12, 20
    dt = torch.float16 if io == "f16" else torch.bfloat16
    x, dy, w, mu1, mu2 = _inputs(3, N, S, F, G, H, W)
    x, dy = (torch.from_numpy(a).to(dt).float().numpy() for a in (x, dy))
    plan = _capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5,
                      flags=_flags(_capi, _capi.FLAG_IO_F16 if io == "f16" else _capi.FLAG_IO_BF16))
    got = run_plan(plan, x, dy, w, mu1, mu2, dtype=dt)
    want = _oracle(("io", io), x, dy, w, mu1, mu2)
    # the storage bars of tests/test_gpu_f16.py and tests/test_gpu_dense_split.py (one rounding to 11 / 8 significant bits)
    rel, floor = (2e-3, 1e-3) if io == "f16" else (2e-2, 4e-3)
    assert_parity(got["y"], want["y"], "pairs-%s/y" % io, rel=rel, floor=floor)
    assert_parity(got["dx"], want["dx"], "pairs-%s/dx" % io, rel=rel, floor=floor)


def _run_raw(plan, x, dy, w, mu1, mu2, dtype=torch.float32, fmt=torch.contiguous_format):
    """forward + backward on tensors of `dtype` in memory format `fmt` -> y, dx as the plan returned them, on the host"""
    dev = lambda a: torch.from_numpy(a).cuda()
    S, G, F = w.shape[1:]
    sg = torch.full((1, S, G, F), 0.5, device="cuda")
    xd, dyd = (dev(a).to(dtype).contiguous(memory_format=fmt) for a in (x, dy))
    y = plan.forward(xd, dev(w), dev(mu1), dev(mu2), sg)
    plan.check_status()
    st = plan.outlier_status()
    dx = plan.backward(xd, dyd, dev(w), dev(mu1), dev(mu2), sg)[0]
    plan.check_status()
    return dict(y=y.cpu(), dx=dx.cpu()), st, plan.outlier_status()


def test_channels_last_activations():
    """S = 40 -> F = 24 (3 / 2 chunks) with x, y, dy, dx in [N][H][W][C]: the fp32 bar, and the bits of the NCHW call of the same
    plan description (the NHWC instantiations share the tap loop and differ in the addresses of their stores)."""
    from dau_conv import _capi
    N, S, F, G, H, W = 2, 40, 24, 2, 12, 20
    x, dy, w, mu1, mu2 = _inputs(3, N, S, F, G, H, W)
    mk = lambda extra: _capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5, flags=_flags(_capi, extra))
    got, _, _ = _run_raw(mk(_capi.FLAG_IO_NHWC), x, dy, w, mu1, mu2, fmt=torch.channels_last)
    ref, _, _ = _run_raw(mk(0), x, dy, w, mu1, mu2)
    want = _oracle(("nhwc", 3), x, dy, w, mu1, mu2)
    for key in ("y", "dx"):
        assert got[key].is_contiguous(memory_format=torch.channels_last)
        assert_parity(got[key].contiguous().numpy(), want[key], "pairs-nhwc/" + key)
        assert torch.equal(got[key].contiguous().view(torch.int32), ref[key].view(torch.int32)), key


def test_outlier_units_join_the_chunk_pair_sums():
    """DAU_FLAG_DENSE_SPLIT_OUTLIERS with three units in (3, 3.99]: the radius-3 GEMM over 3 / 2 chunks whose epilogue adds the ring
    pass's fp32 sums.  The fp32 bar against the oracle; and the float16 plan stores the binary16 rounding of what the fp32 plan
    stores on the same (widened) inputs, bit for bit -- the sums join in fp32 and the store rounds once."""
    from dau_conv import _capi
    N, S, F, G, H, W = 2, 40, 24, 2, 12, 20
    x, dy, w, mu1, mu2 = _inputs(3, N, S, F, G, H, W)
    mu1.flat[7] = 3.4; mu2.flat[7] = -3.99; mu2.flat[S * G * F - 3] = 3.7; mu1.flat[S * G * F // 2] = -3.01
    x, dy = (a.astype(np.float16).astype(np.float32) for a in (x, dy))
    mk = lambda extra: _capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5,
                                  flags=_flags(_capi, _capi.FLAG_DENSE_SPLIT_OUTLIERS | extra))
    ref, st_f, st_b = _run_raw(mk(0), x, dy, w, mu1, mu2)
    assert st_f == (3, True) and st_b == (3, True), (st_f, st_b)
    want = _oracle(("outliers", 3), x, dy, w, mu1, mu2)
    got, st_f, st_b = _run_raw(mk(_capi.FLAG_IO_F16), x, dy, w, mu1, mu2, dtype=torch.float16)
    assert st_f == (3, True) and st_b == (3, True), (st_f, st_b)
    for key in ("y", "dx"):
        assert_parity(ref[key].numpy(), want[key], "pairs-outliers/" + key)
        assert torch.equal(got[key].view(torch.int16), ref[key].to(torch.float16).view(torch.int16)), key


@pytest.mark.parametrize("name", ["S16-F40", "S40-F32", "S7-F5"])
def test_odd_chunk_counts_in_a_poisoned_workspace(name):
    """The workspace (staged planes, dense kernel, everything between and behind them) holds NaN patterns before the call: a read of
    an absent chunk's rows or window would reach an output."""
    from dau_conv import _capi
    s = SHAPES[name]
    N, S, F, G, H, W = (s[q] for q in ("N", "S", "F", "G", "H", "W"))
    x, dy, w, mu1, mu2 = _inputs(3, N, S, F, G, H, W)
    inputs = dict(x=x, dy=dy, w=w, mu1=mu1, mu2=mu2, sigma=np.full_like(w, 0.5))
    plan = _capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5, flags=_flags(_capi))
    want = _oracle((name, 3), x, dy, w, mu1, mu2)
    for fill in (0xFF, 0x7F):
        f = aa.forward(_capi, plan, inputs, fill=fill)
        b = aa.backward(_capi, plan, inputs, fill=fill)
        for rep, key in ((f, "y"), (b, "dx")):
            assert rep.rc == _capi.DAU_OK
            rep.assert_clean("%s/%s/fill %02x" % (name, key, fill))
            assert_parity(rep.values[key], want[key], "pairs-poison/%s/%s" % (name, key))


@pytest.mark.parametrize("S,channel", [(40, 35), (24, 16), (7, 6)])
def test_reach_of_a_non_finite_input_in_the_unpaired_chunk(S, channel):
    """An Inf in a channel of the last, unpaired chunk: the non-finite outputs are exactly those of the 32x32x16 build of the same
    call (the outputs of its own image whose taps touch it), and the finite ones meet the bar."""
    from dau_conv import _capi
    partner = variant_capi("mfma32")
    N, F, G, H, W = 2, 24, 2, 12, 20
    x, dy, w, mu1, mu2 = _inputs(3, N, S, F, G, H, W)
    xn = x.copy()
    xn[1, channel, 5, 7] = np.inf
    ys = []
    for capi in (_capi, partner):
        plan = capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=0.5, flags=_flags(capi))
        dev = lambda a: torch.from_numpy(a).cuda()
        sg = torch.full((1, S, G, F), 0.5, device="cuda")
        ys.append(plan.forward(dev(xn), dev(w), dev(mu1), dev(mu2), sg).cpu().numpy())
        plan.check_status()
    bad = ~np.isfinite(ys[0])
    assert bad.any() and not bad[0].any()
    assert np.array_equal(bad, ~np.isfinite(ys[1]))
    want = _oracle(("inf", S), x, dy, w, mu1, mu2)["y"]
    viol = np.abs(ys[0] - want) - (1e-4 * np.abs(want) + 1e-6 * np.abs(want).max())
    assert viol[~bad].max() <= 0
