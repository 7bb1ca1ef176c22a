"""CPU: sd_xk_walk_kernel in the built gfx950 code (as test_split_dot_stage_built_code.py looks at the other staging kernels of the
two-limb f16 gather-dot).  The release library holds both instantiations -- the maxima pass and the storing pass -- for the
prefilter supports 5, 7 and 9; none touches scratch or spills a VGPR; the storing pass writes XS with 16-byte stores only, and the
maxima pass writes nothing but its atomic maxima."""
import os
import re
import tempfile

from test_built_code import PKG, _kernel_name, _metadata, release  # noqa: F401  (release: the fixture)
from test_split_dot_stage_built_code import _named

SUPPORTS = (5, 7, 9)


def _walk(release, store):
    found = {}
    for sym, ins in _named(release, "sd_xk_walk_kernel").items():
        m = re.search(r"sd_xk_walk_kernel<(\d+), (true|false)>", _kernel_name(sym))
        assert m, _kernel_name(sym)
        if (m.group(2) == "true") == store:
            found[int(m.group(1))] = (sym, ins)
    return found


def test_release_library_holds_both_instantiations_per_support(release):
    assert len(_named(release, "sd_xk_walk_kernel")) == 2 * len(SUPPORTS)
    assert sorted(_walk(release, True)) == sorted(_walk(release, False)) == sorted(SUPPORTS)


def test_walking_kernels_touch_no_scratch(release):
    so = os.path.join(PKG, "libdau_conv_hip.so")
    with tempfile.TemporaryDirectory() as d:
        meta = _metadata(so, d)
    for sym, ins in _named(release, "sd_xk_walk_kernel").items():
        name, m = _kernel_name(sym), meta[sym]
        print("%s: %d VGPRs, scratch %d B, %d spilled VGPRs, %d spilled SGPRs" % (name[:60], m["vgpr"], m["scratch"], m["vgpr_spill"], m["sgpr_spill"]))
        assert not [mn for mn, _ in ins if mn.startswith("scratch_")], name
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)


def test_storing_pass_stores_16_bytes_per_lane_only(release):
    for k, (sym, ins) in _walk(release, True).items():
        stores = {mn for mn, _ in ins if mn.startswith(("global_store", "flat_store", "buffer_store"))}
        assert stores == {"global_store_dwordx4"}, (k, stores)
        assert not [mn for mn, _ in ins if "atomic" in mn], k


def test_maxima_pass_stores_nothing(release):
    for k, (sym, ins) in _walk(release, False).items():
        assert not [mn for mn, _ in ins if mn.startswith(("global_store", "flat_store", "buffer_store"))], k
        assert "global_atomic_umax" in [mn for mn, _ in ins], k
