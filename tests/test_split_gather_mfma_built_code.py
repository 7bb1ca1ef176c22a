"""CPU: the shipped split_gather_kernel instantiations (k_dense_split.hip: the two-limb f16 gather-sum), disassembled as
test_bf16_split_dot_built_code.py does for the gather-dot.  At a radius whose tap loop runs a PAIR of 16-channel chunks per
step, every MFMA is v_mfma_f32_16x16x32_f16; the loop over rows of taps holds six MFMAs (hi.hi, lo.hi, hi.lo for two channel
halves) per (tap, group of 16 pixels), i.e. three per B fragment read from LDS; nothing between the first and the last MFMA
touches scratch, and the kernel keeps two waves per SIMD (at most 256 registers, none spilled).  The other radii, and every radius
of the A/B partner library (-DDAU_SPLIT_MFMA32), keep v_mfma_f32_32x32x16_f16."""
import os
import re
import tempfile

import pytest

from test_built_code import PKG, _code_objects, _functions, _kernel_name, _metadata, release  # noqa: F401  (release: the fixture)
from test_split_dot_built_code import _blocks_that_loop
from util import variant_lib

K32 = "v_mfma_f32_16x16x32_f16"
K16 = "v_mfma_f32_32x32x16_f16"
SWITCHED = ("s3",)        # namespaces (radii) whose tap loop is the chunk-pair form


def _kernels(funcs):
    return {sym: ins for sym, ins in funcs.items() if "split_gather_kernel" in sym}


def _radius(sym):
    return re.search(r"dau::(s\d)::", _kernel_name(sym)).group(1)


def _mfmas(ins):
    return [mn for mn, _ in ins if mn.startswith("v_mfma")]


def test_every_radius_runs_one_mfma_shape(release):
    kernels = _kernels(release)
    assert {_radius(s) for s in kernels} == {"s2", "s3", "s4"}
    for sym, ins in kernels.items():
        want = K32 if _radius(sym) in SWITCHED else K16
        assert set(_mfmas(ins)) == {want}, (_kernel_name(sym), sorted(set(_mfmas(ins))))


def test_tap_row_loop_of_the_chunk_pair_form(release):
    kernels = {s: i for s, i in _kernels(release).items() if _radius(s) in SWITCHED}
    assert kernels
    for sym, ins in kernels.items():
        name = _kernel_name(sym)
        loops = [(a, b) for a, b in _blocks_that_loop(ins) if any(mn.startswith("v_mfma") for mn, _ in ins[a:b])]
        # the loop over rows of taps: the straight-line block with the most MFMAs (tall tiles: one per column half, the same rule for both)
        a, b = max(loops, key=lambda ab: len(_mfmas(ins[ab[0]:ab[1]])))
        body = ins[a:b]
        mfma, reads = len(_mfmas(body)), sum(1 for mn, _ in body if mn == "ds_read_b128")
        print("%s: tap-row loop %d MFMAs, %d ds_read_b128" % (name, mfma, reads))
        assert mfma and mfma % 3 == 0, (name, mfma)
        assert reads * 3 == mfma, (name, reads, mfma)
        mf = [i for i, (mn, _) in enumerate(ins) if mn.startswith("v_mfma")]
        assert not [mn for mn, _ in ins[mf[0]:mf[-1]] if mn.startswith("scratch_")], name


def test_two_waves_per_simd_and_no_spills():
    so = os.path.join(PKG, "libdau_conv_hip.so")
    if not os.path.exists(so):
        pytest.skip("library not built")
    with tempfile.TemporaryDirectory() as d:
        meta = {s: m for s, m in _metadata(so, d).items() if "split_gather_kernel" in s and _radius(s) in SWITCHED}
    assert meta
    for sym, m in meta.items():
        assert m["vgpr"] <= 256 and m["vgpr_spill"] == 0, (_kernel_name(sym), m)


def test_partner_library_keeps_the_32x32x16_loop(release):
    so = variant_lib("mfma32")
    if not os.path.exists(so):
        pytest.skip("library not built")
    with tempfile.TemporaryDirectory() as d:
        funcs = {}
        for co in _code_objects(so, d):
            funcs.update(_functions(co))
    partner = _kernels(funcs)
    assert sorted(partner) == sorted(_kernels(release))
    for sym, ins in partner.items():
        assert set(_mfmas(ins)) == {K16}, _kernel_name(sym)
