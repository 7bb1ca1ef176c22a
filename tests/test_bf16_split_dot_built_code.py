"""CPU: the shipped sd_e1_dot_kernel instantiations (k_split_dot.hip: the split gather-dot with the error in one binary16 limb,
for bfloat16 activations), disassembled as test_split_dot_built_code.py does for the three-product kernel.  Per tile and K step
the kernel runs two MFMAs (hi_x * e, lo_x * e) instead of three: 32 per pair of K steps (x two input channels x four units),
still with at most four global_load_dwordx4 per pair (the A operand is loaded once per pair of K steps), and no scratch access
anywhere between its first and last MFMA."""
import re

from test_built_code import _kernel_name, release  # noqa: F401  (release: the fixture)
from test_split_dot_built_code import _blocks_that_loop

MFMAS_PER_PAIR = 32      # two K steps x two input channels x four units x two limb products


def _kernels(funcs):
    return {sym: ins for sym, ins in funcs.items() if "sd_e1_dot_kernel" in sym}


def test_the_two_region_widths_ship(release):
    names = sorted(_kernel_name(s) for s in _kernels(release))
    assert len(names) == 2 and all(re.search(r"sd_e1_dot_kernel<1[02]>", n) for n in names), names
    assert not [n for n in names if "split_gather_dot_kernel" in n]      # (that name counts the three-product kernels)


def test_no_scratch_between_the_mfmas(release):
    kernels = _kernels(release)
    assert kernels
    for sym, ins in kernels.items():
        mf = [i for i, (mn, _) in enumerate(ins) if mn.startswith("v_mfma")]
        inside = [mn for mn, _ in ins[mf[0]:mf[-1]]]
        assert not [mn for mn in inside if mn.startswith("scratch_")], _kernel_name(sym)


def test_k_loop_runs_two_products_per_tile(release):
    kernels = _kernels(release)
    assert kernels
    for sym, ins in kernels.items():
        name = _kernel_name(sym)
        # the K loop: the straight-line block that ends in a conditional branch and holds the most MFMAs
        a, b = max(_blocks_that_loop(ins), key=lambda ab: sum(1 for mn, _ in ins[ab[0]:ab[1]] if mn.startswith("v_mfma")))
        body = ins[a:b]
        mfma = sum(1 for mn, _ in body if mn.startswith("v_mfma"))
        loads = sum(1 for mn, _ in body if mn == "global_load_dwordx4")
        reads = sum(1 for mn, _ in body if mn == "ds_read_b128")
        print("%s: K loop body %d MFMAs, %d global_load_dwordx4, %d ds_read_b128" % (name, mfma, loads, reads))
        assert mfma and mfma % MFMAS_PER_PAIR == 0, (name, mfma)
        pairs = mfma // MFMAS_PER_PAIR
        assert loads <= 4 * pairs, (name, loads, pairs)
        assert reads == 16 * pairs, (name, reads, pairs)       # one B fragment per tile and K step (the hi limb only)
        assert not [mn for mn, _ in body if mn.startswith("scratch_")], name
