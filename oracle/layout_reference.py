"""Plain numpy references of the data-layout kernels of csrc/conv3x3.hip: the weight images (mtbc_conv3x3_pack_fwd / _pack_dgrad /
_pack_lp / _pack_many), the weight views (mtbc_conv3x3_weight_view / _many) and the channel-blocked 16-bit activation layout
(mtbc_c8_pack / _pack16 / _unpack).  No device, no torch.  Written from the layout descriptions of include/mtbc.h and DESIGN.md.

Every function is a SCATTER: it walks the SOURCE elements -- (co, ci, tap) of a weight, (n, c, px) of an activation -- and places each
into a zero-initialised destination.  The kernels are gathers (one thread per destination piece), so a slip in one index formula is not
repeated here by transcription.  tests/test_layout_reference_cpu.py checks these functions on their own (independent gather decoders,
the meaning of the images as matrix operands of the convolution, hand-written rounding patterns).

These kernels move or round values and add nothing: results are compared as integers.  Values travel as bit patterns (uint32 / uint16
views), so NaN payloads and the sign of zero survive the index arithmetic.

    weight w                  (Cout, Cin, 3, 3) float32, tap = 3 * ky + kx
    fp32 forward image        [ceil(Cout/16)][Cin][9][16]             img[co // 16][ci][tap][co % 16]     = w[co][ci][tap]
    fp32 dgrad image          [ceil(Cin/16)][Cout][9][16]             img[ci // 16][co][8 - tap][ci % 16] = w[co][ci][tap]
    16-bit image              [ceil(rows/16)][ceil(red/32)][9][16][32]; forward: row = co, k = ci, tap; dgrad: row = ci, k = co, 8 - tap;
                              inside the 64-byte row i = row % 16 the 16-byte piece kq = (k % 32) // 8 sits at position kq ^ ((i >> 1) & 3)
    view, mode 0              dst (Cout, cnt, 3, 3):  dst[co][ci - off][tap] = w[co][ci][tap]            for off <= ci < off + cnt
    view, mode 1              dst (cnt, K, 3, 3):     dst[ci - off][k_off + co][8 - tap] = w[co][ci][tap]
    channel-blocked           [N][C/8][HW][8]:        y[n][c // 8][px][c % 8] = x[n][c][px]
"""
import numpy as np

# (Cout, Cin) of the weight-image cases: exact tiles, one past a tile and a chunk, ragged rows, a ragged last chunk, three and more
# chunks, 9 Cin a multiple of 16 and not, the stem.  Shared by the CPU self-checks and the device tests.
PACK_CASES = [(16, 16), (24, 1), (24, 24), (7, 13), (17, 33), (40, 16), (48, 72), (32, 64), (5, 40), (96, 288),
              # the smallest shapes of the benchmark's step programs whose (ragged rows, ragged K, chunks) the ten above do not have:
              # forward full rows / ragged K / 2 chunks, ragged / ragged / 3, ragged / full / 3, full / full / 1; dgrad full / full / 2
              (48, 48), (24, 72), (24, 96), (16, 32), (64, 32)]

# (Cout, Cin, off, cnt, mode, k_off, K) of the weight-view cases; k_off = K = 0 for mode 0
WVIEW_CASES = [
    (5, 12, 0, 4, 0, 0, 0),            # mode 0, a slice at the start; 180 elements: less than one block
    (6, 10, 3, 4, 0, 0, 0),            # in the middle
    (24, 144, 24, 24, 0, 0, 0),        # in the middle, several blocks
    (24, 144, 48, 96, 0, 0, 0),        # at the end
    (7, 9, 0, 9, 0, 0, 0),             # cnt == Cin; 567 elements: a ragged last block
    (24, 48, 0, 24, 1, 0, 40),         # mode 1, k_off == 0 and K > Cout
    (24, 48, 24, 16, 1, 0, 40),        # the same from the middle of the channels
    (16, 16, 0, 16, 1, 0, 40),         # the same over all channels
    (24, 48, 0, 24, 1, 8, 40),         # 0 < k_off and k_off + Cout < K
    (24, 40, 8, 24, 1, 8, 40),         # the same from the middle of the channels
    (48, 96, 0, 48, 1, 8, 56),         # k_off + Cout == K
    (24, 72, 24, 24, 1, 8, 32),
    (96, 288, 96, 96, 1, 8, 104),
    (8, 24, 16, 8, 1, 3, 11),          # the last channels into the last K
]

# (N, C, HW, strided).  strided: the source is channels [8, 8 + C) of a 40-channel tensor, src_batch_stride = 40 HW
C8_PACK_CASES = [(1, 8, 1, False), (3, 24, 120, False), (2, 8, 300, False), (2, 16, 77, False), (2, 16, 128, False), (2, 16, 77, True), (3, 16, 120, True)]
C8_PACK16_CASES = [(1, 8, 4, False), (3, 24, 36, False), (2, 16, 260, False), (2, 16, 512, False), (2, 16, 260, True), (3, 16, 36, True)]


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ sizes
def packed_elems(Cin, Cout):
    return cdiv(Cout, 16) * Cin * 9 * 16


def packed_dgrad_elems(Cin, Cout):
    return cdiv(Cin, 16) * Cout * 9 * 16


def packed_lp_elems(Cin, Cout, dgrad):
    rows, red = (Cin, Cout) if dgrad else (Cout, Cin)
    return cdiv(rows, 16) * cdiv(red, 32) * 9 * 16 * 32


# ------------------------------------------------------------------ rounding
def round16(x, compute):
    """float32 -> the 16-bit pattern (uint16) of compute 1 = bf16 / 2 = fp16, round to nearest even.  NaN -> a quiet NaN of the same sign."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if compute == 2:
        with np.errstate(over="ignore", under="ignore", invalid="ignore"):
            return x.astype(np.float16).view(np.uint16)
    assert compute == 1, compute
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)          # add half an ulp of the kept part, less one when it is even
    nan = (u & 0x7fffffff) > 0x7f800000
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def widen16(h, compute):
    """uint16 patterns of bf16 / fp16 -> the float32 they stand for (exact)."""
    h = np.ascontiguousarray(h, dtype=np.uint16)
    if compute == 2:
        return h.view(np.float16).astype(np.float32)
    assert compute == 1, compute
    return (h.astype(np.uint32) << 16).view(np.float32)


def is_nan16(h, compute):
    h = np.asarray(h, dtype=np.uint16)
    return (h & 0x7fff) > (0x7c00 if compute == 2 else 0x7f80)


# ------------------------------------------------------------------ weight images
def _source(w):
    """(bit patterns (Cout, Cin, 9), co, ci, tap index grids over the source)"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    Cout, Cin = w.shape[:2]
    co, ci, tap = np.meshgrid(np.arange(Cout), np.arange(Cin), np.arange(9), indexing="ij")
    return w.view(np.uint32).reshape(Cout, Cin, 9), co, ci, tap


def pack_fwd(w):
    u, co, ci, tap = _source(w)
    Cout, Cin = u.shape[:2]
    img = np.zeros((cdiv(Cout, 16), Cin, 9, 16), np.uint32)
    img[co // 16, ci, tap, co % 16] = u
    return img.view(np.float32)


def pack_dgrad(w):
    u, co, ci, tap = _source(w)
    Cout, Cin = u.shape[:2]
    img = np.zeros((cdiv(Cin, 16), Cout, 9, 16), np.uint32)
    img[ci // 16, co, 8 - tap, ci % 16] = u
    return img.view(np.float32)


def pack_lp(w, dgrad, compute):
    _, co, ci, tap = _source(w)
    Cout, Cin = co.shape[:2]
    h = round16(w, compute).reshape(Cout, Cin, 9)
    row, k, t = (ci, co, 8 - tap) if dgrad else (co, ci, tap)
    rows, red = (Cin, Cout) if dgrad else (Cout, Cin)
    img = np.zeros((cdiv(rows, 16), cdiv(red, 32), 9, 16, 32), np.uint16)
    i, kk = row % 16, k % 32
    piece = (kk // 8) ^ ((i >> 1) & 3)
    img[row // 16, k // 32, t, i, piece * 8 + kk % 8] = h
    return img


def weight_view(w, off, cnt, mode, k_off, K, dst):
    """Writes the view into dst -- float32, (Cout, cnt, 3, 3) for mode 0, (cnt, K, 3, 3) for mode 1 -- and leaves the rest of it alone."""
    u, co, ci, tap = _source(w)
    Cout = u.shape[0]
    assert dst.dtype == np.float32 and dst.flags.c_contiguous and dst.shape == ((cnt, K, 3, 3) if mode else (Cout, cnt, 3, 3)), dst.shape
    sel = (ci >= off) & (ci < off + cnt)
    u, co, ci, tap = u[sel], co[sel], ci[sel], tap[sel]
    d = dst.view(np.uint32).reshape(dst.shape[0], dst.shape[1], 9)
    if mode:
        d[ci - off, k_off + co, 8 - tap] = u
    else:
        d[co, ci - off, tap] = u
    return dst


# ------------------------------------------------------------------ channel-blocked activations
def _blocked(v):
    """(N, C, HW) -> [N][C/8][HW][8], any 2- or 4-byte words."""
    N, C, HW = v.shape
    assert C % 8 == 0, C
    n, c, px = np.meshgrid(np.arange(N), np.arange(C), np.arange(HW), indexing="ij")
    y = np.zeros((N, C // 8, HW, 8), v.dtype)
    y[n, c // 8, px, c % 8] = v
    return y


def c8_pack(x, compute):
    """float32 (N, C, HW) -> uint16 [N][C/8][HW][8] of the type of `compute`."""
    return _blocked(round16(x, compute))


def c8_pack16(x16):
    """uint16 (N, C, HW) -> the same words as [N][C/8][HW][8]."""
    return _blocked(np.ascontiguousarray(x16, dtype=np.uint16))


def c8_unpack(y, compute):
    """uint16 [N][C/8][HW][8] -> float32 (N, C, HW), exact."""
    y = np.ascontiguousarray(y, dtype=np.uint16)
    N, G, HW, _ = y.shape
    n, g, px, e = np.meshgrid(np.arange(N), np.arange(G), np.arange(HW), np.arange(8), indexing="ij")
    x = np.zeros((N, G * 8, HW), np.uint32)
    x[n, g * 8 + e, px] = widen16(y, compute).view(np.uint32)
    return x.view(np.float32)


# ------------------------------------------------------------------ the values that go wrong in a conversion
def _f(bits):
    return [b & 0xffffffff for b in bits]


# float32 bit patterns.  both formats: +-0, +-inf, NaN, +-1e-45 (the smallest fp32 subnormal)
SPECIAL_COMMON = _f([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x00000001, 0x80000001])
# bf16, by the 16 dropped bits: 0x8000 above an even result (tie, down), 0x8000 above an odd result (tie, up), 0x7fff, 0x8001, a carry into
# the exponent, the largest finite fp32 (-> inf); and their negatives
_BF = [0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x3fffffff, 0x7f7fffff]
SPECIAL_BF16 = _f(_BF + [b | 0x80000000 for b in _BF])
# fp16: 65504, 65519.996, 65520 (tie -> inf), 2^-24, 2^-25 (tie -> 0), nextafter(2^-25, 1), 3 x 2^-25 (tie -> 2^-23), 16.5 x 2^-24 (tie -> 16) and
# the same with a sticky bit (-> 17); and their negatives
_FP = [0x477fe000, 0x477fefff, 0x477ff000, 0x33800000, 0x33000000, 0x33000001, 0x33c00000, 0x35840000, 0x35840001]
SPECIAL_F16 = _f(_FP + [b | 0x80000000 for b in _FP])


def specials(compute):
    """float32 array of the special values a source of the type of `compute` (0: fp32 images, the common list) carries."""
    bits = SPECIAL_COMMON + (SPECIAL_BF16 if compute == 1 else SPECIAL_F16 if compute == 2 else SPECIAL_BF16 + SPECIAL_F16)
    return np.array(bits, dtype=np.uint32).view(np.float32)


def plant(x, compute, must=()):
    """Overwrites a scattered set of elements of the float32 array x (in place, flat order) with specials(compute), one value at each flat
    index of `must` first, the others 1 + 7 j (mod size) apart.  Returns x."""
    assert x.dtype == np.float32 and x.flags.c_contiguous
    flat = x.reshape(-1)
    sp = specials(compute)
    where = list(must)
    j = 0
    while len(where) < len(must) + len(sp) and j < flat.size:
        p = (1 + 7 * j) % flat.size
        if p not in where:
            where.append(p)
        j += 1
    for n, p in enumerate(where):
        flat[p] = sp[n % len(sp)]
    return x


def weight_edges(Cout, Cin):
    """Flat indices into a (Cout, Cin, 3, 3) weight that lie in the last row of the last row tile and the last K of the last chunk, for the
    forward image (row = co, K = ci) and for the dgrad image (row = ci, K = co): the last output channel and the last input channel."""
    idx = lambda co, ci, tap: (co * Cin + ci) * 9 + tap      # noqa: E731
    return sorted({idx(Cout - 1, 0, 4), idx(0, Cin - 1, 2), idx(Cout - 1, Cin - 1, 8), idx(Cout - 1, Cin // 2, 0), idx(Cout // 2, Cin - 1, 6)})
