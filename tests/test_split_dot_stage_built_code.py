"""CPU: the staging kernels of the two-limb f16 gather-dot in the built gfx950 code (as test_split_dot_built_code.py looks at
the main kernel).  max |Xk| is taken inside blur4_pack_kernel<K, true>, so the release library holds no sd_absmax_x_kernel
(only the stage_ref build of `make tuning` keeps it, with the earlier sd_stage_e_kernel); the new sd_stage_e_kernel and the
blur4_pack_kernel instantiations, with and without the maxima, touch no scratch."""
import os
import re
import tempfile

import pytest

from test_built_code import PKG, _code_objects, _functions, _kernel_name, _metadata, release  # noqa: F401  (release: the fixture)
from util import variant_lib


def _named(funcs, part):
    return {sym: ins for sym, ins in funcs.items() if part in sym}


def test_release_library_has_no_pass_of_its_own_for_the_xk_maxima(release):
    assert not [_kernel_name(s) for s in _named(release, "sd_absmax_x_kernel")]
    assert len(_named(release, "sd_absmax_e_kernel")) == 1            # (its neighbour is found: the names match)


def test_stage_ref_build_keeps_the_earlier_staging():
    so = variant_lib("stage_ref")
    if not os.path.exists(so):
        pytest.skip("libraries not built")
    with tempfile.TemporaryDirectory() as d:
        funcs = {}
        for co in _code_objects(so, d):
            funcs.update(_functions(co))
    assert len(_named(funcs, "sd_absmax_x_kernel")) == 1
    # the earlier sd_stage_e_kernel uses no LDS; the new one transposes through it
    stage = list(_named(funcs, "sd_stage_e_kernel").values())
    assert len(stage) == 1 and not [mn for mn, _ in stage[0] if mn.startswith("ds_")]


def test_staging_kernels_touch_no_scratch(release):
    so = os.path.join(PKG, "libdau_conv_hip.so")
    with tempfile.TemporaryDirectory() as d:
        meta = _metadata(so, d)
    stage = _named(release, "sd_stage_e_kernel")
    blur4 = _named(release, "blur4_pack_kernel")
    names = sorted(_kernel_name(s) for s in blur4)
    assert len(stage) == 1
    # supports 7, 5, 9 and any (0), each with and without the maxima
    assert len(names) == 8 and sum(1 for n in names if re.search(r"blur4_pack_kernel<\d, true>", n)) == 4, names
    for sym, ins in list(stage.items()) + list(blur4.items()):
        name = _kernel_name(sym)
        m = meta[sym]
        # (SGPR spills go to VGPR lanes, not to scratch: the 9-tap instantiations keep 54 taps in scalar registers)
        print("%s: %d VGPRs, scratch %d B, %d spilled VGPRs, %d spilled SGPRs" % (name[:60], m["vgpr"], m["scratch"], m["vgpr_spill"], m["sgpr_spill"]))
        assert not [mn for mn, _ in ins if mn.startswith("scratch_")], name
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)


def test_new_error_staging_stores_whole_runs(release):
    """one 16-byte global store per lane and iteration, fed by one ds_read_b128 (the transpose), 16-byte LDS writes"""
    (ins,) = _named(release, "sd_stage_e_kernel").values()
    mns = [mn for mn, _ in ins]
    assert "ds_read_b128" in mns and "ds_write_b128" in mns and "global_store_dwordx4" in mns
    assert not [mn for mn in mns if re.match(r"global_store_(byte|short|dword|dwordx2)$", mn)], mns
    assert "global_atomic_umax" in [mn for mn, _ in next(iter(_named(release, "blur4_pack_kernelILi7ELb1").values()))]
