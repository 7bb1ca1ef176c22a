"""CPU: the walking sd_stage_e_kernel (k_split_dot.hip: the error staging of the two-limb f16 gather-dot) in the built gfx950 code,
read from the code objects' metadata as test_split_stage_walk_built_code.py reads the gather-sum's.  The release library holds it as
ONE kernel whose body is instantiated for the three activation formats (with_act: float32, bfloat16 and float16 loads all appear in
its code); it touches no scratch, spills no vector register and stays within the 168 registers of three waves per SIMD (its two row
images of 8 KiB leave room for ten waves per CU).  Its stores are 16-byte pieces fed by 16-byte LDS reads.  The stage_e_rows variant
(-DDAU_SD_STAGE_E_ROWS) holds the workgroup-per-window-row kernel and not the walking one; the stage_ref variant the oldest form."""
import os
import tempfile

import pytest

import util
from test_built_code import PKG, _code_objects, _functions, _kernel_name, _metadata

THREE_WAVES = 168         # registers per lane at three waves per SIMD


def _stage_e(so):
    """{demangled name: (metadata, instructions)} of the sd_stage_e_kernel symbols of a library"""
    if not os.path.exists(so):
        pytest.skip("library not built")
    with tempfile.TemporaryDirectory() as d:
        meta = _metadata(so, d)
        funcs = {}
        for co in _code_objects(so, d):
            funcs.update(_functions(co))
    return {_kernel_name(sym): (meta[sym], funcs[sym]) for sym in meta if "sd_stage_e_kernel" in sym}


def test_release_ships_the_walking_kernel_for_every_format_without_scratch():
    kernels = _stage_e(os.path.join(PKG, "libdau_conv_hip.so"))
    assert len(kernels) == 1, sorted(kernels)
    (name, (m, ins)), = kernels.items()
    assert "SeWalkArgs" in name, name
    print("%s: %d VGPRs, %d bytes of scratch, %d spilled VGPRs, %d SGPRs kept in VGPR lanes" % (name, m["vgpr"], m["scratch"], m["vgpr_spill"], m["sgpr_spill"]))
    assert m["scratch"] == 0 and m["vgpr_spill"] == 0, m
    assert 0 < m["vgpr"] <= THREE_WAVES, m
    mns = [mn for mn, _ in ins]
    assert not [mn for mn in mns if mn.startswith("scratch_")]
    # float32 rows are dword loads, bfloat16 and float16 rows 16-bit loads (two bodies of them): 32 loads per row and body
    assert mns.count("global_load_dword") >= 32 and mns.count("global_load_ushort") >= 2 * 32, (mns.count("global_load_dword"), mns.count("global_load_ushort"))
    assert "ds_write_b128" in mns and "ds_read_b128" in mns and "global_store_dwordx4" in mns


def test_the_rows_variant_holds_the_row_kernel_and_not_the_walking_one():
    kernels = _stage_e(util.variant_lib("stage_e_rows"))
    assert len(kernels) == 1, sorted(kernels)
    (name, (m, ins)), = kernels.items()
    assert "SeWalkArgs" not in name, name
    mns = [mn for mn, _ in ins]
    assert "ds_write_b128" in mns and "ds_read_b128" in mns and "s_barrier" in mns     # the LDS transpose of a 256-thread workgroup
    assert m["scratch"] == 0 and m["vgpr_spill"] == 0, m


def test_the_reference_variant_keeps_the_oldest_form():
    kernels = _stage_e(util.variant_lib("stage_ref"))
    assert len(kernels) == 1, sorted(kernels)
    (name, (m, ins)), = kernels.items()
    assert "SeWalkArgs" not in name and not [mn for mn, _ in ins if mn.startswith("ds_")], name
