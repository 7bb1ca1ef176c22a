"""CPU: the shipped split_gather_dot_kernel instantiations (k_split_dot.hip), disassembled as in test_built_code.py.  The A
operand is loaded once per pair of K steps and the odd step's fragment is built with quad-permute DPP moves: the K loop's body
must hold at most four global_load_dwordx4 per two K steps (48 MFMAs; the per-step loads had eight), DPP moves, and no scratch
access anywhere between the kernel's first and last MFMA.  (The body spans two pairs, one per register set: 96 MFMAs, so at
most eight loads.)"""
import re

from test_built_code import _kernel_name, release  # noqa: F401  (release: the fixture)

MFMAS_PER_PAIR = 48      # two K steps x two input channels x four units x three limb products


def _kernels(funcs):
    return {sym: ins for sym, ins in funcs.items() if "split_gather_dot_kernel" in sym}


def _blocks_that_loop(ins):
    """(begin, end) instruction indices of the straight-line blocks that end in a conditional branch (llvm-objdump names a
    branch target by offset, not by label, so loop bodies are recognised as such blocks; the K loop is the one with the MFMAs)"""
    cuts = [-1] + [i for i, (mn, _) in enumerate(ins) if mn.startswith(("s_cbranch", "s_branch", "s_barrier", "s_endpgm"))]
    return [(a + 1, b) for a, b in zip(cuts, cuts[1:]) if ins[b][0].startswith("s_cbranch")]


def test_the_two_region_widths_ship(release):
    names = sorted(_kernel_name(s) for s in _kernels(release))
    assert len(names) == 2 and all(re.search(r"split_gather_dot_kernel<1[02]>", n) for n in names), names


def test_no_scratch_between_the_mfmas(release):
    for sym, ins in _kernels(release).items():
        mf = [i for i, (mn, _) in enumerate(ins) if mn.startswith("v_mfma")]
        inside = [mn for mn, _ in ins[mf[0]:mf[-1]]]
        assert not [mn for mn in inside if mn.startswith("scratch_")], _kernel_name(sym)


def test_k_loop_loads_each_column_pair_once(release):
    for sym, ins in _kernels(release).items():
        name = _kernel_name(sym)
        # the K loop: the straight-line block that ends in a conditional branch and holds the most MFMAs
        a, b = max(_blocks_that_loop(ins), key=lambda ab: sum(1 for mn, _ in ins[ab[0]:ab[1]] if mn.startswith("v_mfma")))
        body = ins[a:b]
        mfma = sum(1 for mn, _ in body if mn.startswith("v_mfma"))
        loads = sum(1 for mn, _ in body if mn == "global_load_dwordx4")
        dpp = sum(1 for mn, ops in body if mn.endswith("_dpp") or "quad_perm" in ops)
        print("%s: K loop body %d MFMAs, %d global_load_dwordx4, %d DPP moves" % (name, mfma, loads, dpp))
        assert mfma and mfma % MFMAS_PER_PAIR == 0, (name, mfma)
        pairs = mfma // MFMAS_PER_PAIR
        assert loads <= 4 * pairs, (name, loads, pairs)
        assert dpp >= 16 * pairs, (name, dpp, pairs)           # 2 channels x 2 limbs x 4 dwords per pair
        assert not [mn for mn, _ in body if mn.startswith("scratch_")], name
