"""oracle/layout_reference.py -- the numpy references the bit-for-bit layout tests of tests/test_ops_gpu.py compare the weight-image, weight-view
and channel-blocking kernels with -- checked on its own, without a device:
  * every image is decoded again by a GATHER over flat offsets written here (the references are scatters over index grids);
  * the decoded fp32 and 16-bit images, read as matrices A[row][k * 9 + tap], reproduce F.conv2d and its input gradient as plain matrix
    products over an im2col in fp64 -- which ties the tap flip and the transpose to the operation and not to a formula;
  * mode-1 views of two consumers side by side are the weight of ONE forward conv that yields the sum of their input gradients;
  * round16 against hand-written bit patterns;
  * the library's size functions and its host-side refusals (they return before any device call)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from multi_task_breast_cancer_amd import _lib as L
from oracle import layout_reference as R


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return L.load()


def _w(Cout, Cin, compute=0, seed=0):
    rng = np.random.default_rng(1993 + 131 * Cout + 17 * Cin + seed)
    w = rng.standard_normal((Cout, Cin, 3, 3)).astype(np.float32)
    return R.plant(w, compute, R.weight_edges(Cout, Cin))


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ decoders: gathers over flat offsets
def _grid(Cout, Cin):
    return np.meshgrid(np.arange(Cout), np.arange(Cin), np.arange(9), indexing="ij")


def _gather(img, offs):
    """(the elements of the flat image at offs, True when every other element is zero)"""
    flat = _bits(img).reshape(-1)
    rest = np.ones(flat.size, bool)
    rest[offs.reshape(-1)] = False
    assert int(rest.sum()) == flat.size - offs.size, "two weights decode from one place"
    return flat[offs], not flat[rest].any()


def decode_fwd(img, Cout, Cin):
    co, ci, t = _grid(Cout, Cin)
    return _gather(img, ((co // 16 * Cin + ci) * 9 + t) * 16 + co % 16)


def decode_dgrad(img, Cout, Cin):
    co, ci, t = _grid(Cout, Cin)
    return _gather(img, ((ci // 16 * Cout + co) * 9 + (8 - t)) * 16 + ci % 16)


def decode_lp(img, Cout, Cin, dgrad):
    co, ci, t = _grid(Cout, Cin)
    if dgrad:
        r, k, t, red = ci, co, 8 - t, Cout
    else:
        r, k, red = co, ci, Cin
    nch = (red + 31) // 32
    i = r % 16
    piece = ((k % 32) >> 3) ^ ((i >> 1) & 3)
    return _gather(img, ((((r // 16 * nch + k // 32) * 9 + t) * 16 + i) * 4 + piece) * 8 + k % 8)


def decode_c8(y, N, Cc, HW):
    n, c, px = np.meshgrid(np.arange(N), np.arange(Cc), np.arange(HW), indexing="ij")
    return _gather(y, ((n * (Cc // 8) + c // 8) * HW + px) * 8 + c % 8)


@pytest.mark.parametrize("Cout,Cin", R.PACK_CASES)
def test_weight_images_decode_to_the_weight_and_pad_with_zero(Cout, Cin):
    w = _w(Cout, Cin)
    u = w.view(np.uint32).reshape(Cout, Cin, 9)
    for name, img, dec, elems in (("fwd", R.pack_fwd(w), decode_fwd, R.packed_elems(Cin, Cout)),
                                  ("dgrad", R.pack_dgrad(w), decode_dgrad, R.packed_dgrad_elems(Cin, Cout))):
        assert img.dtype == np.float32 and img.size == elems, name
        got, clean = dec(img, Cout, Cin)
        assert np.array_equal(got, u), name
        assert clean, f"{name}: padding not zero"
    for compute in (1, 2):
        w = _w(Cout, Cin, compute)
        h = R.round16(w, compute).reshape(Cout, Cin, 9)
        for dgrad in (0, 1):
            img = R.pack_lp(w, dgrad, compute)
            assert img.dtype == np.uint16 and img.size == R.packed_lp_elems(Cin, Cout, dgrad), (compute, dgrad)
            got, clean = decode_lp(img, Cout, Cin, dgrad)
            assert np.array_equal(got, h), (compute, dgrad)
            assert clean, f"16-bit image compute {compute} dgrad {dgrad}: padding not zero"


@pytest.mark.parametrize("N,Cc,HW", sorted({c[:3] for c in R.C8_PACK_CASES + R.C8_PACK16_CASES}))
def test_channel_blocked_layout_decodes_and_unpacks(N, Cc, HW):
    rng = np.random.default_rng(7 + N + Cc + HW)
    for compute in (1, 2):
        x = R.plant(rng.standard_normal((N, Cc, HW)).astype(np.float32) * 3, compute, [N * Cc * HW - 1])
        h = R.round16(x, compute)
        y = R.c8_pack(x, compute)
        assert y.shape == (N, Cc // 8, HW, 8) and y.dtype == np.uint16
        got, clean = decode_c8(y, N, Cc, HW)
        assert np.array_equal(got, h) and clean
        assert np.array_equal(R.c8_pack16(h), y)
        back = R.c8_unpack(y, compute)
        want = R.widen16(h, compute)
        ok = ~np.isnan(want)
        assert back.shape == x.shape and np.array_equal(np.isnan(back), ~ok) and np.array_equal(back.view(np.uint32)[ok], want.view(np.uint32)[ok])
        # widening is exact: rounding the unpacked values again changes nothing
        assert np.array_equal(R.round16(back, compute)[ok], h[ok])


# ------------------------------------------------------------------ what the images mean
def _im2col(x):
    """(C, H, W) float64 -> (C * 9, H * W): row c * 9 + tap holds x[c] shifted by tap = 3 ky + kx, zero outside (pad 1)."""
    Cc, H, W = x.shape
    xp = np.zeros((Cc, H + 2, W + 2))
    xp[:, 1:-1, 1:-1] = x
    col = np.zeros((Cc, 9, H, W))
    for ky in range(3):
        for kx in range(3):
            col[:, 3 * ky + kx] = xp[:, ky:ky + H, kx:kx + W]
    return col.reshape(Cc * 9, H * W)


def _fwd_matrix(img, rows, red):
    """A[r][k * 9 + tap] of an fp32 image [tile][k][tap][16]."""
    a = np.asarray(img, dtype=np.float64).reshape(-1, red, 9, 16)
    return a.transpose(0, 3, 1, 2).reshape(-1, red * 9)[:rows]


def _lp_matrix(img, rows, red, compute):
    """A[r][k * 9 + tap] of a 16-bit image [tile][chunk][tap][16 rows][4 pieces][8]: piece `pos` of row i holds K group pos ^ ((i >> 1) & 3)."""
    T, Ch = img.shape[:2]
    a = R.widen16(img, compute).astype(np.float64).reshape(T, Ch, 9, 16, 4, 8)
    out = np.zeros((T * 16, Ch * 32, 9))
    for t in range(T):
        for c in range(Ch):
            for i in range(16):
                for pos in range(4):
                    k0 = c * 32 + (pos ^ ((i >> 1) & 3)) * 8
                    out[t * 16 + i, k0:k0 + 8, :] = a[t, c, :, i, pos, :].T
    assert not out[rows:].any() and not out[:, red:].any()
    return out[:rows, :red].reshape(rows, red * 9)


@pytest.mark.parametrize("Cout,Cin", [(7, 13), (17, 33), (24, 1), (40, 16)])
def test_images_are_the_matrix_operands_of_the_convolution(Cout, Cin):
    H, W = 5, 6
    g = torch.Generator().manual_seed(11 * Cout + Cin)
    x = torch.randn(1, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    dz = torch.randn(1, Cout, H, W, generator=g, dtype=torch.float64)
    rng = np.random.default_rng(Cout + Cin)
    w32 = rng.standard_normal((Cout, Cin, 3, 3)).astype(np.float32)
    for compute in (0, 1, 2):
        if compute:
            wv = R.widen16(R.round16(w32, compute), compute)           # the stored weight
            a_f = _lp_matrix(R.pack_lp(w32, 0, compute), Cout, Cin, compute)
            a_d = _lp_matrix(R.pack_lp(w32, 1, compute), Cin, Cout, compute)
        else:
            wv = w32
            a_f = _fwd_matrix(R.pack_fwd(w32), Cout, Cin)
            a_d = _fwd_matrix(R.pack_dgrad(w32), Cin, Cout)
        z = F.conv2d(x, torch.from_numpy(wv.astype(np.float64)), padding=1)
        dx, = torch.autograd.grad(z, x, dz)
        got_z = a_f @ _im2col(x.detach().numpy()[0])
        got_dx = a_d @ _im2col(dz.numpy()[0])
        assert np.abs(got_z - z.detach().numpy()[0].reshape(Cout, -1)).max() <= 1e-12 * float(z.detach().abs().max()), compute
        assert np.abs(got_dx - dx.numpy()[0].reshape(Cin, -1)).max() <= 1e-12 * float(dx.abs().max()), compute


def test_mode1_views_side_by_side_are_the_weight_of_the_gathered_dgrad():
    """Two 3x3 consumers read channels [off, off + cnt) of one tensor.  Their mode-1 views at k_off 0 and Cout_a of one (cnt, K, 3, 3) tensor,
    used as the weight of a FORWARD conv over cat(dz_a, dz_b), give the sum of the two input gradients of that channel range."""
    H, W, cnt = 5, 6, 6
    rng = np.random.default_rng(3)
    g = torch.Generator().manual_seed(3)
    cons = [(5, 10, 4), (7, 6, 0)]              # (Cout, Cin, off)
    K = sum(c[0] for c in cons)
    dst = np.full((cnt, K, 3, 3), 1993.0, np.float32)
    want = torch.zeros(1, cnt, H, W, dtype=torch.float64)
    dzs, k_off = [], 0
    for Cout, Cin, off in cons:
        w = rng.standard_normal((Cout, Cin, 3, 3)).astype(np.float32)
        R.weight_view(w, off, cnt, 1, k_off, K, dst)
        x = torch.randn(1, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
        dz = torch.randn(1, Cout, H, W, generator=g, dtype=torch.float64)
        dx, = torch.autograd.grad(F.conv2d(x, torch.from_numpy(w.astype(np.float64)), padding=1), x, dz)
        want += dx[:, off:off + cnt]
        dzs.append(dz)
        k_off += Cout
    got = F.conv2d(torch.cat(dzs, 1), torch.from_numpy(dst.astype(np.float64)), padding=1)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("case", R.WVIEW_CASES, ids=lambda c: "-".join(map(str, c)))
def test_weight_view_reference_against_slicing(case):
    """mode 0 is w[:, off:off + cnt]; mode 1 is that slice with the two channel axes swapped and the taps reversed, at [:, k_off:k_off + Cout];
    everything else of the destination keeps its pre-fill."""
    Cout, Cin, off, cnt, mode, k_off, K = case
    w = _w(Cout, Cin)
    dst = np.full((cnt, K, 3, 3) if mode else (Cout, cnt, 3, 3), 1993.0, np.float32)
    R.weight_view(w, off, cnt, mode, k_off, K, dst)
    want = np.full(dst.shape, 1993.0, np.float32)
    sl = w[:, off:off + cnt]
    if mode:
        want[:, k_off:k_off + Cout] = sl.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
    else:
        want[...] = sl
    assert _same_bits(dst, want)


# ------------------------------------------------------------------ rounding: hand-written patterns
# float32 bits -> (bf16 bits, fp16 bits); None: not in that format's list
ROUND16_BY_HAND = {
    0x00000000: (0x0000, 0x0000), 0x80000000: (0x8000, 0x8000),          # +-0
    0x7f800000: (0x7f80, 0x7c00), 0xff800000: (0xff80, 0xfc00),          # +-inf
    0x7fc00000: ("nan", "nan"),
    0x00000001: (0x0000, 0x0000), 0x80000001: (0x8000, 0x8000),          # +-1e-45 -> +-0
    # bf16: 1.0 + dropped bits
    0x3f808000: (0x3f80, None),      # tie above the even 0x3f80: down
    0x3f818000: (0x3f82, None),      # tie above the odd 0x3f81: up
    0x3f807fff: (0x3f80, None),      # just below the tie
    0x3f808001: (0x3f81, None),      # just above the tie
    0x3fffffff: (0x4000, None),      # 1.9999999 -> 2.0: the carry runs into the exponent
    0x7f7fffff: (0x7f80, None),      # the largest finite fp32 -> inf
    # fp16
    0x477fe000: (None, 0x7bff),      # 65504, the largest finite fp16
    0x477fefff: (None, 0x7bff),      # 65519.996
    0x477ff000: (None, 0x7c00),      # 65520: tie between 65504 (odd) and 2^16 -> inf
    0x33800000: (None, 0x0001),      # 2^-24, the smallest subnormal
    0x33000000: (None, 0x0000),      # 2^-25: tie between 0 and 2^-24 -> 0
    0x33000001: (None, 0x0001),      # nextafter(2^-25, 1)
    0x33c00000: (None, 0x0002),      # 3 x 2^-25: tie between 1 and 2 (x 2^-24) -> 2^-23
    0x35840000: (None, 0x0010),      # 16.5 x 2^-24: tie -> 16
    0x35840001: (None, 0x0011),      # the same with a sticky bit -> 17
}


def test_round16_on_the_special_values():
    for compute, extra in ((1, R.SPECIAL_BF16), (2, R.SPECIAL_F16)):
        bits = np.array(R.SPECIAL_COMMON + extra, dtype=np.uint32)
        assert np.array_equal(R.specials(compute).view(np.uint32), bits)
        got = R.round16(bits.view(np.float32), compute)
        for b, h in zip(bits.tolist(), got.tolist()):
            want = ROUND16_BY_HAND[b][compute - 1] if b in ROUND16_BY_HAND else ROUND16_BY_HAND[b & 0x7fffffff][compute - 1] | 0x8000
            assert want is not None, hex(b)
            if want == "nan":
                assert bool(R.is_nan16(np.uint16(h), compute)), (hex(b), hex(h))
            else:
                assert h == want, (compute, hex(b), hex(h), hex(want))
    # the values are what their comments say
    f = lambda b: float(np.array([b], np.uint32).view(np.float32)[0])      # noqa: E731
    assert f(0x477fe000) == 65504.0 and f(0x477ff000) == 65520.0 and f(0x33800000) == 2.0 ** -24 and f(0x33c00000) == 3 * 2.0 ** -25
    assert f(0x33000001) == float(np.nextafter(np.float32(2.0 ** -25), np.float32(1))) and f(0x35840000) == 16.5 * 2.0 ** -24
    assert f(0x00000001) == float(np.float32(1e-45)) and f(0x7f7fffff) == float(np.finfo(np.float32).max)
    # torch's CPU conversions round the same way (NaN aside)
    x = np.random.default_rng(5).standard_normal(4096).astype(np.float32) * np.float32(10.0) ** np.random.default_rng(6).integers(-9, 6, 4096).astype(np.float32)
    for compute in (1, 2):
        t = torch.from_numpy(np.concatenate([x, R.specials(compute)]))
        ref = (t.bfloat16() if compute == 1 else t.half()).view(torch.int16).numpy().view(np.uint16)
        got = R.round16(t.numpy(), compute)
        ok = ~np.isnan(t.numpy())
        assert np.array_equal(got[ok], ref[ok])


def test_plant_puts_specials_on_the_ragged_edges():
    for Cout, Cin in R.PACK_CASES:
        for compute in (1, 2):
            w = _w(Cout, Cin, compute).reshape(Cout, Cin, 9)
            plain = np.random.default_rng(1993 + 131 * Cout + 17 * Cin).standard_normal((Cout, Cin, 9)).astype(np.float32)
            changed = w.view(np.uint32) != plain.view(np.uint32)
            assert changed[Cout - 1].any() and changed[:, Cin - 1].any(), (Cout, Cin)          # the last row and the last K of both images


# ------------------------------------------------------------------ the library's host-only answers
def test_size_functions_equal_the_reference(lib):
    for Cout, Cin in R.PACK_CASES + [c[:2] for c in R.WVIEW_CASES]:
        assert lib.mtbc_conv3x3_packed_elems(Cin, Cout) == R.packed_elems(Cin, Cout), (Cout, Cin)
        assert lib.mtbc_conv3x3_packed_dgrad_elems(Cin, Cout) == R.packed_dgrad_elems(Cin, Cout), (Cout, Cin)
        for dgrad in (0, 1):
            assert lib.mtbc_conv3x3_packed_lp_elems(Cin, Cout, dgrad) == R.packed_lp_elems(Cin, Cout, dgrad), (Cout, Cin, dgrad)


BADSHAPE, BADARG = -1, -2
_P = [C.c_void_p(i << 20) for i in range(1, 4)]          # aligned non-null pointers nothing dereferences: every call below returns first


def test_layout_entry_points_refuse_on_the_host(lib):
    """The codes returned today for arguments the layout kernels cannot take, all before any device call."""
    src, dst = _P[0], _P[1]
    assert lib.mtbc_c8_pack(src, 12 * 16, dst, 2, 12, 16, 1, None) == BADSHAPE                 # C % 8
    assert lib.mtbc_c8_unpack(src, dst, 2, 12, 16, 1, None) == BADSHAPE
    assert lib.mtbc_c8_pack(src, 8 * 16, dst, 2, 8, 16, 0, None) == BADARG                     # fp32 has no channel-blocked form
    assert lib.mtbc_c8_pack16(src, 8 * 6, dst, 2, 8, 6, None) == BADSHAPE                      # HW % 4
    assert lib.mtbc_c8_pack16(src, 8 * 16 + 2, dst, 2, 8, 16, None) == BADARG                  # source batch stride % 4
    assert lib.mtbc_c8_pack16(src, 12 * 16, dst, 2, 12, 16, None) == BADSHAPE                  # C % 8
    # a view past the input channels, a mode-1 view past K: BADARG from the single call, BADSHAPE from the batched one
    for bad in ((24, 48, 40, 16, 0, 0, 0), (24, 48, 0, 24, 1, 20, 40), (24, 48, -1, 8, 0, 0, 0), (24, 48, 0, 24, 1, -1, 40)):
        assert lib.mtbc_conv3x3_weight_view(src, dst, *bad, None) == BADARG, bad
        d = (L.WViewDesc * 1)()
        d[0].w, d[0].dst = src.value, dst.value
        d[0].Cout, d[0].Cin, d[0].ci_off, d[0].ci_cnt, d[0].mode, d[0].k_off, d[0].K = bad
        assert lib.mtbc_conv3x3_weight_view_many(d, 1, None) == BADSHAPE, bad
    assert lib.mtbc_conv3x3_weight_view(src, dst, 24, 48, 0, 24, 2, 0, 0, None) == BADARG      # mode
    # an unknown kind, a 16-bit kind without a 16-bit format
    for kind, compute in ((4, 1), (-1, 0), (2, 0), (3, 0), (3, 3)):
        d = (L.PackDesc * 1)()
        d[0].w, d[0].packed, d[0].Cin, d[0].Cout, d[0].kind, d[0].compute = src.value, dst.value, 24, 24, kind, compute
        assert lib.mtbc_conv3x3_pack_many(d, 1, None) == BADARG, (kind, compute)
    assert lib.mtbc_conv3x3_pack_lp(src, dst, 24, 24, 0, 0, None) == BADARG
    assert lib.mtbc_conv3x3_pack_many(None, 0, None) == 0 and lib.mtbc_conv3x3_pack_many(None, 1, None) == BADARG
