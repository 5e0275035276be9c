"""The device-only leaves the kernels are built from, one by one: the cross-lane primitives of csrc/lh_wave.h, the two
scans of lh_dev_common.h, the DPP control words the code base uses, the hand-written band sums of lh_dev_qloop.h and the
math leaves of lh_dev_math.h / lh_dev_psy_core.h / lh_dev_qloop.h.  These are the pieces the CPU emulator replaces with
plain C under LH_EMU, so the emulator tests never see the code that ships; the end-to-end parity tests reach them only
through whatever values a synthetic signal happens to put into them.

tests/gpu_tools/lh_leaf_kernels.hip applies one leaf per lane per case and writes every lane's result; all comparison
happens here, against references in numpy (tests/leaf_support.py).  Every GPU test has a CPU twin that runs the same
cases through the emulator build of the same drivers (libhipemu_leaf.so): it proves the cases, the references and the
fixtures on a machine without a GPU.  A failure names the leaf, the case, the wave and lane, and gives both values in hex.

Wave primitives: 128 threads = two waves with different data, full EXEC, both waves checked.  Every primitive gets 32
cases of random full-range words, all zero, all ones, all lanes equal, a single non-zero lane at 0 / 15 / 16 / 31 / 32 /
47 / 48 / 63 and the lane index as the value (leaf_support.word_families); the float maxima get both signs, +-0,
subnormals and +-FLT_MAX instead (float_families; no NaN, which is their contract); lh_bcast_u32 every source lane,
lh_shfl_* self / reversal / all-from-one, lh_wave_sum_regions its fields at their maxima 127 and 255.

Math leaves whose authority is the libm of the reference build (glibc 2.35): tests/golden/leaf_math_sha256.json holds one
sha256 per sweep (tests/golden/make_leaf_math_golden.py).  On the CPU: libm here == host-compiled leaf == committed
digest; on the device: sha256 of the device's output == committed digest, and the host-compiled leaf locates a mismatch.
"""
import pytest

import leaf_support as ls

gpu = pytest.mark.gpu

# which case calls which function of the device half of lh_wave.h: leaf_support.WORDS (the keys are the parameters below)
WAVE_PARAMS = ls.WAVE_OPS


# ------------------------------------------------------------------------------------------------ wave primitives
@pytest.mark.parametrize("op", WAVE_PARAMS)
def test_wave_primitive_emulated(op):
    assert ls.check_wave("emu", op) >= 44


@gpu
@pytest.mark.parametrize("op", WAVE_PARAMS)
def test_wave_primitive_on_device(op):
    assert ls.check_wave("gpu", op) >= 44


def test_dpp_control_words_cover_the_ones_the_code_uses():
    """the list of the issue: lh_dpp with 0xB1, 0x4E, 0x141, 0x140, 0x111, 0x112, 0x113, 0x114, 0x118, 0x128, 0x104, 0x130,
    0x138; lh_dpp_rows with 0x142 / 0xa and 0x143 / 0xc"""
    plain = {c for _, c, m, _ in ls.DPP_SLOTS if m == 0xf}
    rows = {(c, m) for _, c, m, _ in ls.DPP_SLOTS if m != 0xf}
    assert plain == {0xB1, 0x4E, 0x141, 0x140, 0x111, 0x112, 0x113, 0x114, 0x118, 0x128, 0x104, 0x130, 0x138}
    assert rows == {(0x142, 0xa), (0x143, 0xc)}
    assert [s for s, _, _, _ in ls.DPP_SLOTS] == list(range(len(ls.DPP_SLOTS))) and len(ls.DPP_SLOTS) <= ls.NOUT


# ------------------------------------------------------------------------------------------------ band sums
@pytest.mark.parametrize("pad", [1, 0], ids=["lq_band_sums_pad", "lq_band_sums"])
def test_band_sum_inputs_discriminate(pad):
    """The conditions on the inputs, in numpy: terms positive (a random mantissa in [1, 4) times one power of two per band);
    dropping the last term or adding one more changes the sum's bits for every lane with n >= 1; a pairwise-tree sum and a
    reversed sum each differ in bits from the serial sum for at least 90 % of the lanes with n >= 8.

    A seed alone does not reach that share: for terms of one size a tree sum of n random terms differs from the serial sum
    in 36 % (n = 8) .. 87 % (n = 192) of bands, a reversed sum in 46 % .. 91 %, and BANDSUM_SEED = 20 as drawn gave 60 % /
    64 % over all such lanes.  So every band with n >= 8 draws its mantissas again, from the same distribution, until both
    other orders show (leaf_support.bandsum_cases).  Measured then: padded layout, tree 100 %, reversed 100 % of 763 such
    lanes; back-to-back layout, tree 100 %, reversed 100 % of 778."""
    tree, rev, lanes = ls.bandsum_discrimination(pad, ls.runner("emu").sq_n)
    print("pad=%d: tree sum differs for %.1f %%, reversed sum for %.1f %% of the %d lanes with n >= 8" % (pad, 100 * tree, 100 * rev, lanes))
    assert tree >= 0.9 and rev >= 0.9


@pytest.mark.parametrize("pad", [1, 0], ids=["lq_band_sums_pad", "lq_band_sums"])
def test_band_sums_emulated(pad):
    assert ls.check_bandsum("emu", pad) >= 11


@gpu
@pytest.mark.parametrize("pad", [1, 0], ids=["lq_band_sums_pad", "lq_band_sums"])
def test_band_sums_on_device(pad):
    """the serial float32 sum in index order, bit for bit; EXEC back for all 128 lanes; maxw as the product forms it"""
    assert ls.check_bandsum("gpu", pad) >= 11


# ------------------------------------------------------------------------------------------------ math leaves
LIBM_SWEEPS = ["powf(10, y)", "powf(x, 0.36)", "powf(x, 0.18)", "powf special cases", "powf thresholds", "logf subnormals",
               "logf normals, 0, inf, 1", "log10f subnormals", "log10f normals, 0, inf, 1", "vbrold_adjust long",
               "vbrold_adjust short", "vbrold_masking_lower"]


def test_libm_sweeps_are_the_committed_ones():
    rec = ls.committed_digests()
    assert sorted(k for k in rec if not k.startswith("_")) == sorted(LIBM_SWEEPS) == sorted(ls.libm_sweeps())
    for name, (_, a, _, _) in ls.libm_sweeps().items():
        assert rec[name]["points"] == a.size <= 1 << 24


@pytest.mark.parametrize("name", LIBM_SWEEPS)
def test_math_leaf_equals_libm_and_digest_on_host(name):
    assert ls.check_libm_sweep_host(name) > 0


@gpu
@pytest.mark.parametrize("name", LIBM_SWEEPS)
def test_math_leaf_equals_digest_on_device(name):
    assert ls.check_libm_sweep_device(name) > 0


OTHER_LEAVES = {"lh_fast_log2 and LH_FAST_LOG2_VIA": ls.check_fast_log2, "lh_mask_add_near and lh_mask_add_far": ls.check_mask_add,
                "lh_ns_interp": ls.check_ns_interp, "lq_ldexp": ls.check_ldexp}


@pytest.mark.parametrize("leaf", list(OTHER_LEAVES))
def test_masking_and_step_leaf_emulated(leaf):
    assert OTHER_LEAVES[leaf]("emu") > 0


@gpu
@pytest.mark.parametrize("leaf", list(OTHER_LEAVES))
def test_masking_and_step_leaf_on_device(leaf):
    assert OTHER_LEAVES[leaf]("gpu") > 0
