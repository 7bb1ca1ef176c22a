"""CPU: the shipped split_stage_walk_kernel instantiations (k_dense_split.hip: the walking form of the two-limb gather-sum's
staging), read from the built code objects' metadata as test_built_code.py reads the hot kernels': every prefilter support
(3, 5, 7, 9, 11) in every activation format and offset radius (namespaces s2, s3, s4) ships, none of them touches scratch or
spills a register, and the supports up to 7 -- the ring of filtered rows and the raw rows in flight fit -- stay within the 128
registers of four waves per SIMD.  The -DDAU_SPLIT_STAGE_REF variant holds none of them."""
import os
import re
import tempfile

import pytest

import util
from test_built_code import PKG, _kernel_name, _metadata

SUPPORTS = (3, 5, 7, 9, 11)
FOUR_WAVES = 128          # registers per lane at four waves per SIMD


def _walk_kernels(so):
    if not os.path.exists(so):
        pytest.skip("library not built")
    with tempfile.TemporaryDirectory() as d:
        meta = _metadata(so, d)
    return {_kernel_name(sym): m for sym, m in meta.items() if "split_stage_walk_kernel" in sym}


def test_every_support_format_and_radius_ships_without_scratch():
    kernels = _walk_kernels(os.path.join(PKG, "libdau_conv_hip.so"))
    seen = set()
    for name, m in sorted(kernels.items()):
        hit = re.search(r"dau::(s\d)::split_stage_walk_kernel<(\d+), (\d+)>", name)
        assert hit, name
        ns, k, act = hit.group(1), int(hit.group(2)), int(hit.group(3))
        seen.add((ns, k, act))
        print("%s: %d VGPRs, %d bytes of scratch, %d SGPRs kept in VGPR lanes" % (name.split("(")[0], m["vgpr"], m["scratch"], m["sgpr_spill"]))
        # (the tap pairs and the uniform addresses do not all fit the scalar registers: the rest sits in lanes of a VGPR, not in memory)
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)
        assert 0 < m["vgpr"] <= (FOUR_WAVES if k <= 7 else 256), (name, m)
    assert seen == {(ns, k, act) for ns in ("s2", "s3", "s4") for k in SUPPORTS for act in (0, 1, 2)}, sorted(seen)


def test_the_reference_variant_holds_no_walking_kernel():
    assert not _walk_kernels(util.variant_lib("split_stage_ref"))
