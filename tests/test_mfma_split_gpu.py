"""The two forms of the chunked kernels' split of fp32 into bf16 hi + lo (csrc/wkv6_chunk.h: the residual lo = x - float(hi) by four v_dot2c
per lane, or by one MFMA with A = -I per wave), side by side on the same inputs through the library's debug entry wkv6_debug_split: rows of
64 lanes x 4 floats, one wave per row.

  * hi: both forms equal RNE_bf16(x), bit for bit, on every input;
  * lo, |x| >= 2^-110: the two forms agree bit for bit, and equal RNE_bf16(x - float(hi)) (the subtraction is exact in fp32) wherever that
    residual is zero or a normal fp32 -- random normals at scales 2^-100 .. 2^100, bf16-exact values (lo = 0), values one fp32 ulp below a
    power of two (hi rounds into the next binade), +-0, the largest values whose hi is finite;
  * the largest finite values proper (hi = Inf): v_dot2c gives lo = -Inf (+Inf for a negative x) in that element and NaN in the other element
    of its packed pair (0 x Inf: the instruction multiplies both halves of the pair); the MFMA gives the same in that element when it is the
    only one of its tile column (lane % 16 of the row), and NaN in the 15 other elements of the column (0 x Inf in the zero entries of -I)
    -- the header's stated behaviour; every element of another column agrees bit for bit;
  * |x| < 2^-110 (values in 2^-126 .. 2^-118, fp32 subnormals): what was measured on the MI355X and written down in profiles/mfma_split.txt:
    nothing is flushed in either form -- hi, and lo down to the bf16 subnormals, agree bit for bit and equal RNE_bf16(x - float(hi))."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LANES, SLOTS = 64, 4


@pytest.fixture(scope="module")
def run():
    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    from rwkv_lm_ext_amd import _lib
    lib = _lib.load()

    def call(x):
        """x: float32 [rows, 64, 4] -> uint16 bit patterns (hi_dot, lo_dot, hi_mfma, lo_mfma), each [rows, 64, 4]"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        rows = x.shape[0]
        assert x.shape == (rows, LANES, SLOTS)
        xd = torch.from_numpy(x).cuda()
        out = torch.zeros(4, rows, LANES, SLOTS, dtype=torch.int16, device="cuda")
        _lib.check(lib.wkv6_debug_split(rows, xd.data_ptr(), out.data_ptr(), None), "wkv6_debug_split")
        torch.cuda.synchronize()
        return tuple(out.cpu().numpy().view(np.uint16))
    return call


def bf16_bits(x):
    """RNE_bf16 of a float32 array, as bit patterns"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def from_bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def finite_inputs():
    """[rows, 64, 4] float32: every class of the docstring whose hi is finite and whose |x| is 0 or >= 2^-110"""
    g = np.random.default_rng(20240611)
    rows = []
    for e in range(-100, 101):                                           # random normals at scales 2^-100 .. 2^100
        rows.append(np.ldexp(g.standard_normal((LANES, SLOTS)), e).astype(np.float32))
    for e in (-100, -50, -1, 0, 1, 50, 100):                            # bf16-exact: lo = 0
        rows.append(bf16_value(bf16_bits(np.ldexp(g.standard_normal((LANES, SLOTS)), e).astype(np.float32))))
    ex = g.integers(-100, 101, size=(8, LANES, SLOTS))                   # one fp32 ulp below a power of two, both signs
    below = np.nextafter(np.ldexp(np.float32(1), ex).astype(np.float32), np.float32(0))
    rows.extend(below * np.where(g.integers(0, 2, size=below.shape) == 1, np.float32(-1), np.float32(1)))
    rows.append(np.where(g.integers(0, 2, size=(LANES, SLOTS)) == 1, np.float32(-0.0), np.float32(0.0)))   # +-0
    top = from_bits(0x7f7f0000 + g.integers(0, 0x8000, size=(4, LANES, SLOTS)))      # the largest values whose hi (0x7f7f) is finite
    top[0, :, 0] = from_bits(0x7f7f7fff)
    rows.extend(top * np.where(g.integers(0, 2, size=top.shape) == 1, np.float32(-1), np.float32(1)))
    return np.stack(rows).astype(np.float32)


def test_both_forms_on_finite_inputs(run):
    x = finite_inputs()
    big = (x == 0) | (np.abs(x) >= 2.0 ** -110)                         # (a normal at scale 2^-100 falls below now and then)
    hd, ld, hm, lm = run(x)
    want_hi = bf16_bits(x)
    assert np.isfinite(bf16_value(want_hi)).all()
    print(f"rows {x.shape[0]}: hi v_dot2c != RNE {np.count_nonzero(hd != want_hi)}, hi MFMA != RNE {np.count_nonzero(hm != want_hi)}, "
          f"lo forms differ {np.count_nonzero(ld != lm)} (of them |x| >= 2^-110: {np.count_nonzero((ld != lm) & big)})")
    assert (hd == want_hi).all() and (hm == want_hi).all()
    assert (ld == lm)[big].all()
    res = x - bf16_value(want_hi)                                        # exact in fp32
    plain = big & ((res == 0) | (np.abs(res) >= 2.0 ** -126))
    want_lo = bf16_bits(res)
    print(f"residuals zero or normal: {np.count_nonzero(plain)} of {plain.size}; lo MFMA != RNE(x - hi) there: "
          f"{np.count_nonzero((lm != want_lo) & plain)}")
    assert (lm == want_lo)[plain].all()
    exact = bf16_value(want_hi) == x                                     # the bf16-exact rows and +-0 among them
    assert exact.any() and ((lm & 0x7fff) == 0)[exact].all()


def test_an_overflowing_hi_spreads_over_its_tile_column_in_the_mfma_form_only(run):
    g = np.random.default_rng(7)
    big = np.finfo(np.float32).max
    x = g.standard_normal((3, LANES, SLOTS)).astype(np.float32)
    x[0, 5, 2] = big                                                     # row 0: one element, lane 5 slot 2 -> column 5
    x[1, 37, 0] = -big                                                   # row 1: one element, lane 37 -> column 5 as well, negative
    x[2] = big * np.where(g.integers(0, 2, size=(LANES, SLOTS)) == 1, np.float32(-1), np.float32(1))   # row 2: every element
    hd, ld, hm, lm = run(x)
    want_hi = bf16_bits(x)
    assert (hd == want_hi).all() and (hm == want_hi).all()
    assert want_hi[0, 5, 2] == 0x7f80 and want_hi[1, 37, 0] == 0xff80
    col5 = (np.arange(LANES) % 16 == 5)
    for row, lane, slot, own in ((0, 5, 2, 0xff80), (1, 37, 0, 0x7f80)):
        others = np.ones((LANES, SLOTS), bool)
        others[lane, slot] = False
        # v_dot2c: x - (+-Inf) in the element itself, 0 x Inf in the other half of its pair, nothing else moves
        nan = np.isnan(bf16_value(ld[row]))
        assert ld[row, lane, slot] == own and nan[lane, slot ^ 1] and np.count_nonzero(nan) == 1
        # the MFMA: the only Inf of its column, -1 x Inf + 15 x (0 x finite) + x; the 15 other elements of tile column 5, 0 x Inf
        nan = np.isnan(bf16_value(lm[row]))
        assert lm[row, lane, slot] == own
        assert nan[col5[:, None] & others].all()
        assert not nan[~col5].any() and (lm[row][~col5] == ld[row][~col5]).all()
    assert np.isnan(bf16_value(ld[2])).all()                             # both halves of every pair are Inf: -1 x Inf + 0 x Inf
    assert np.isnan(bf16_value(lm[2])).all()                             # every column holds an Inf


def tiny_inputs():
    """[rows, 64, 4] float32 below 2^-110: normals in 2^-126 .. 2^-118 and fp32 subnormals, both signs"""
    g = np.random.default_rng(99)
    sign = lambda shape: np.where(g.integers(0, 2, size=shape) == 1, np.float32(-1), np.float32(1))
    rows = []
    for e in range(-126, -117):
        m = 1 + g.random((LANES, SLOTS))
        rows.append(np.ldexp(m, e).astype(np.float32) * sign((LANES, SLOTS)))
    sub = from_bits(g.integers(1, 0x800000, size=(6, LANES, SLOTS)))                 # subnormals: exponent field 0
    sub[0, :, 0] = from_bits(1)
    sub[0, :, 1] = from_bits(0x7fffff)
    rows.extend(sub * sign(sub.shape))
    return np.stack(rows).astype(np.float32)


def test_tiny_values_as_measured(run):
    """|x| < 2^-110.  Measured on the MI355X (profiles/mfma_split.txt): neither form flushes anything -- of 2304 normals in 2^-126 .. 2^-118
    and 1536 fp32 subnormals, hi and lo of both forms equal RNE_bf16(x) and RNE_bf16(x - float(hi)) in every element, the residuals that are
    fp32 subnormals and round to bf16 subnormals included (516 / 1536 of the residuals round to zero, in the reference as well)."""
    x = tiny_inputs()
    assert (np.abs(x) < 2.0 ** -110).all()
    hd, ld, hm, lm = run(x)
    want_hi = bf16_bits(x)
    res = x - bf16_value(want_hi)
    want_lo = bf16_bits(res)
    normal = np.abs(x) >= 2.0 ** -126
    for name, m in (("normals 2^-126 .. 2^-118", normal), ("fp32 subnormals", ~normal)):
        print(f"{name}: {np.count_nonzero(m)} elements; hi v_dot2c != RNE {np.count_nonzero((hd != want_hi) & m)}, hi MFMA != RNE "
              f"{np.count_nonzero((hm != want_hi) & m)}, hi forms differ {np.count_nonzero((hd != hm) & m)}; lo forms differ "
              f"{np.count_nonzero((ld != lm) & m)}, lo v_dot2c != RNE(x - hi) {np.count_nonzero((ld != want_lo) & m)}, lo MFMA != RNE(x - hi) "
              f"{np.count_nonzero((lm != want_lo) & m)}, lo v_dot2c zero {np.count_nonzero(((ld & 0x7fff) == 0) & m)}, lo MFMA zero "
              f"{np.count_nonzero(((lm & 0x7fff) == 0) & m)}, RNE(x - hi) zero {np.count_nonzero(((want_lo & 0x7fff) == 0) & m)}")
    assert (hd == want_hi).all() and (hm == want_hi).all()
    assert (ld == lm).all() and (lm == want_lo).all()
    sub_lo = ((lm & 0x7f80) == 0) & ((lm & 0x7f) != 0)                   # residuals kept as bf16 subnormals: the case is really there
    assert sub_lo.any()
