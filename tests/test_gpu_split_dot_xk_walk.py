"""GPU: the x side of the two-limb f16 gather-dot's staging (k_split_dot.hip).  NCHW plans whose prefilter support is instantiated
(5, 7, 9) write XS straight from x with the two instantiations of sd_xk_walk_kernel -- one pass for max |Xk|, one that filters
again, scales, splits and stores -- instead of blur4_pack_kernel -> fp32 XK -> sd_stage_x_kernel.  The sums run in blur4_pack's
order and the maxima are taken over the same values, so the four parameter gradients must be BIT-IDENTICAL (0 differing words) to
the build that keeps the XK chain for every plan (libdau_conv_hip_xk_copy.so of `make tuning`: -DDAU_SD_XK_COPY).

Which chain a plan takes follows from its shape alone (sd_walks, k_split_dot.hip): walking kernels for NCHW activations and a
support of 5, 7 or 9, the XK chain for everything else (NHWC; wider supports never reach this member).  Every case asserts the
support its plan reports (Plan.info["blur_support"]) and with it the chain it exercises; the NHWC case is the fallback.  The
walking kernels take a map of any width in column tiles of 16, so there is no width beyond them to test: the 90-wide map runs six
tiles, the 13x11 one a single partial tile.

Cases, the smallest at which each part can go wrong: two octets with one image in the second, odd N, a ragged channel block, a map
that is no multiple of 4 rows or of a region width; region width 10 with one partial octet; the flagship geometry (56x56, region
width 12); supports 5 and 9; float16 and bfloat16 activations; an Inf and a NaN in one input channel; a workspace full of 0xFF bytes
(every XS byte the main kernel reads is written by the call)."""
import os

import numpy as np
import pytest

from util import make_inputs, region_width, variant_capi, variant_lib

pytestmark = pytest.mark.gpu

PARAMS = ("dw", "dmu1", "dmu2", "dsigma")
WALK_SUPPORTS = (5, 7, 9)
FIRST = (9, 5, 3, 4, 13, 11)


def _partner():
    if not os.path.exists(variant_lib("xk_copy")):
        pytest.skip("libraries not built")
    return variant_capi("xk_copy")


def _inputs(seed, shape):
    N, S, F, G, H, W = shape
    x, dy, w, mu1, mu2 = make_inputs(seed, N, S, F, G, H, W, 9, 3.0)
    mu1.flat[0] = 3.0; mu2.flat[0] = -3.0; mu1.flat[1] = -3.0; mu2.flat[1] = 3.0
    return x, dy, w, mu1, mu2


def _gradients(capi, tensors, sigma=0.5, extra=(), support=7, fill=None):
    """The four parameter gradients (numpy) of one backward call; extra: names of plan flags; fill: byte the workspace holds before"""
    import torch
    x, dy, w, mu1, mu2 = tensors
    N, S, H, W = x.shape
    G, F = w.shape[2:]
    flags = capi.FLAG_USE_INTERPOLATION | capi.FLAG_DENSE_SPLIT_F16 | sum(getattr(capi, f) for f in extra)
    plan = capi.Plan(N, S, F, G, H, W, max_kernel_size=9, sigma_hint=sigma, flags=flags)
    assert plan.info["blur_support"] == support, plan.info
    dtype = torch.float16 if "FLAG_IO_F16" in extra else torch.bfloat16 if "FLAG_IO_BF16" in extra else torch.float32
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    act = lambda a: dev(a).to(dtype).contiguous(memory_format=torch.channels_last if "FLAG_IO_NHWC" in extra else torch.contiguous_format)
    sg = torch.full((1, S, G, F), float(sigma), device="cuda")
    if fill is not None:
        plan._workspace(capi.PASS_BACKWARD, torch.device("cuda", torch.cuda.current_device())).fill_(fill)
    need = capi.NEED_DW | capi.NEED_DMU1 | capi.NEED_DMU2 | capi.NEED_DSIGMA
    g = plan.backward(act(x), act(dy), dev(w), dev(mu1), dev(mu2), sg, need_mask=need)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in zip(("dx",) + PARAMS, g) if k in PARAMS}


def _assert_same_bits(name, new, ref):
    for key in PARAMS:
        a, b = np.ascontiguousarray(new[key]).view(np.uint32), np.ascontiguousarray(ref[key]).view(np.uint32)
        differ = int((a != b).sum())
        print("%s/%s: %d of %d words differ" % (name, key, differ, a.size))
        assert differ == 0, "%s/%s: %d words differ" % (name, key, differ)


CASES = [
    # name, (N, S, F, G, H, W), region width, sigma, prefilter support, extra plan flags, chain of the shipped build
    ("ragged", FIRST, 12, 0.5, 7, (), "walk"),
    ("width-10-partial-octet", (3, 16, 16, 2, 27, 27), 10, 0.5, 7, (), "walk"),
    ("flagship-geometry", (8, 16, 16, 2, 56, 56), 12, 0.5, 7, (), "walk"),
    ("support-5", FIRST, 12, 0.4, 5, (), "walk"),
    ("support-9", FIRST, 12, 0.8, 9, (), "walk"),
    ("six-column-tiles", (2, 4, 16, 2, 6, 90), 12, 0.5, 7, (), "walk"),
    ("f16-io", FIRST, 12, 0.5, 7, ("FLAG_IO_F16",), "walk"),
    ("bf16-io", FIRST, 12, 0.5, 7, ("FLAG_IO_BF16",), "walk"),
    ("nhwc-fallback", FIRST, 12, 0.5, 7, ("FLAG_IO_NHWC",), "copy"),
]


@pytest.mark.parametrize("name,shape,rw,sigma,support,extra,chain", CASES, ids=[c[0] for c in CASES])
def test_walking_kernels_are_bit_identical_to_the_xk_chain(name, shape, rw, sigma, support, extra, chain):
    from dau_conv import _capi
    partner = _partner()
    assert region_width(shape[5]) == rw
    # sd_walks: the chain this case exercises in the shipped build
    assert chain == ("walk" if support in WALK_SUPPORTS and "FLAG_IO_NHWC" not in extra else "copy")
    tensors = _inputs(1401 + rw + support, shape)
    new = _gradients(_capi, tensors, sigma, extra, support)
    ref = _gradients(partner, tensors, sigma, extra, support)
    for key in PARAMS:
        assert np.all(np.isfinite(new[key])) and np.abs(new[key]).max() > 0, key
    _assert_same_bits(name, new, ref)


def test_an_inf_and_a_nan_in_one_input_channel():
    """Inf and NaN in input channel 3 of x, one of them in the last, unpaired image (whose absent partner blur4_pack fills with
    0 * value): every gradient word, the NaN ones included, is the XK chain's, and the other input channels stay finite"""
    from dau_conv import _capi
    partner = _partner()
    x, dy, w, mu1, mu2 = _inputs(1411, FIRST)
    x[8, 3, 6, 5] = np.inf
    x[2, 3, 2, 9] = np.nan
    new = _gradients(_capi, (x, dy, w, mu1, mu2))
    ref = _gradients(partner, (x, dy, w, mu1, mu2))
    _assert_same_bits("non-finite", new, ref)
    others = [s for s in range(FIRST[1]) if s != 3]
    for key in PARAMS:
        assert np.all(np.isfinite(new[key][:, others])), key
    assert not np.all(np.isfinite(new["dw"][:, 3]))


def test_every_staged_byte_the_main_kernel_reads_is_written():
    """the workspace full of 0xFF bytes before the call against a zeroed one: the zero row and column in front of XS, those behind
    the image and the absent images of the partial octet are stores of the walking kernel, not leftovers"""
    from dau_conv import _capi
    tensors = _inputs(1421, FIRST)
    poisoned = _gradients(_capi, tensors, fill=0xFF)
    zeroed = _gradients(_capi, tensors, fill=0)
    for key in PARAMS:
        assert np.all(np.isfinite(poisoned[key])), key
    _assert_same_bits("poisoned-workspace", poisoned, zeroed)
