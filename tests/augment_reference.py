"""numpy oracle of ryolo_letterbox_augment, written from the definition (include/ryolo.h), not from the kernel.
Reads the fp32 parameter rows as given; evaluates every stage in float64 (default) or in float32 (the operations the kernel executes,
for measuring how far fp32 rounding alone moves a result).  The noise hash is integer arithmetic and exact in both.
Values are on the 0..255 scale until augment() divides by 255; nothing is quantised in between."""
import numpy as np

MAX_BLUR_SIGMA = 1.5
RADIUS = 4


def _mix(h):
    h = h.astype(np.uint32)
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x7feb352d)
    h = h ^ (h >> np.uint32(15))
    h = h * np.uint32(0x846ca68b)
    h = h ^ (h >> np.uint32(16))
    return h


def noise_bits(seed, n, H, W):
    """(r1, r2): the two 32-bit words of every output pixel of batch slot n, uint32 [H, W]"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over='ignore'):
        k = _mix(np.array([(seed + 0x9e3779b9) & 0xFFFFFFFF], dtype=np.uint32))
        k = _mix(k ^ np.uint32(seed >> 32))
        k = _mix(k ^ np.uint32(n))
        ky = _mix(k ^ np.arange(H, dtype=np.uint32))                          # [H]
        kxy = _mix(ky[:, None] ^ np.arange(W, dtype=np.uint32)[None, :])      # [H, W]
        return _mix(kxy + np.uint32(0x9e3779b9)), _mix(kxy + np.uint32(0x3c6ef372))


def normal(seed, n, H, W, dtype=np.float64):
    """Box-Muller z of every output pixel"""
    r1, r2 = noise_bits(seed, n, H, W)
    f = dtype
    u1 = ((r1 >> np.uint32(8)).astype(np.int64) + 1).astype(f) * f(2.0 ** -24)
    u2 = (r2 >> np.uint32(8)).astype(f) * f(2.0 ** -24)
    two_pi = f(np.float32(6.2831853071795865))      # the kernel's fp32 constant, in either precision
    return np.sqrt(f(-2.0) * np.log(u1)) * np.cos(two_pi * u2)


def sample(img, row, H, W, dtype=np.float64):
    """stage 1: bilinear through the row's matrix, taps outside the source = 128 -> [H, W, 3]"""
    f = dtype
    h, w = img.shape[:2]
    m = [f(v) for v in row[:6]]
    x = np.arange(W, dtype=f)[None, :]
    y = np.arange(H, dtype=f)[:, None]
    sx = (m[0] * x + m[1] * y) + m[2]
    sy = (m[3] * x + m[4] * y) + m[5]
    inside = (sx > -1) & (sx < w) & (sy > -1) & (sy < h)
    sx, sy = np.where(inside, sx, f(-1)), np.where(inside, sy, f(-1))
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0f)[..., None], (sy - y0f)[..., None]
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    padded = np.full((h + 2, w + 2, 3), 128, dtype=f)
    padded[1:-1, 1:-1] = img.astype(f)

    def tap(ix, iy):
        return padded[iy + 1, ix + 1]

    one = f(1)
    v = (one - fy) * ((one - fx) * tap(x0, y0) + fx * tap(x0 + 1, y0)) + fy * ((one - fx) * tap(x0, y0 + 1) + fx * tap(x0 + 1, y0 + 1))
    return np.where(inside[..., None], v, f(128))


def _reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    t = np.mod(i, period)
    return np.where(t < n, t, period - t)


def blur_weights(sigma, dtype=np.float64):
    f = dtype
    s = min(f(sigma), f(MAX_BLUR_SIGMA))
    d = np.arange(-RADIUS, RADIUS + 1)
    with np.errstate(divide='ignore', invalid='ignore', under='ignore'):
        g = np.exp(-(d * d).astype(f) / (f(2) * s * s)).astype(f)
    g[RADIUS] = 1
    total = f(0)
    for v in g:
        total = f(total + v)
    return (g / total).astype(f)


def blur(v, sigma, dtype=np.float64):
    """stage 4 on an [H, W, 3] array: rows, then columns, BORDER_REFLECT_101 (a halo value IS the value at the reflected pixel)"""
    f = dtype
    H, W = v.shape[:2]
    wgt = blur_weights(sigma, f)
    ys = _reflect101(np.arange(-RADIUS, H + RADIUS), H)
    xs = _reflect101(np.arange(-RADIUS, W + RADIUS), W)
    ext = v[ys][:, xs]                                       # [H + 8, W + 8, 3]
    hp = np.zeros((H + 2 * RADIUS, W, 3), dtype=f)
    for d in range(2 * RADIUS + 1):
        hp = (hp + wgt[d] * ext[:, d:d + W]).astype(f)
    out = np.zeros((H, W, 3), dtype=f)
    for d in range(2 * RADIUS + 1):
        out = (out + wgt[d] * hp[d:d + H]).astype(f)
    return out


def satval(v, sat, val, dtype=np.float64):
    """stage 5: the hue-free closed form"""
    f = dtype
    M = v.max(2, keepdims=True)
    m = v.min(2, keepdims=True)
    V = np.minimum(f(val) * M, f(255))
    with np.errstate(divide='ignore', invalid='ignore'):
        S = np.minimum(f(sat) * (M - m) / M, f(1))
        c = V * (f(1) - S * (M - v) / (M - m))
    c = np.where(M == m, V, c)
    return np.where(M <= 0, f(0), c).astype(f)


def stages(img, row, seed, n, H, W, dtype=np.float64):
    """all stages of one batch slot on the 0..255 scale, before the output clamp -> [H, W, 3]"""
    f = dtype
    noise, gamma, gmax, bsig, sat, val, alpha = [f(v) for v in row[6:13]]
    v = sample(img, row, H, W, f)
    if noise != 0:
        v = np.clip(v + (noise * normal(seed, n, H, W, f))[..., None], f(0), f(255))
    if gamma != 1 and gmax > 0:
        v = np.power(v / gmax, gamma) * gmax
    if bsig > 0:
        v = blur(v, bsig, f)
    if sat != 1 or val != 1:
        v = satval(v, sat, val, f)
    if alpha != 0:
        L = (f(np.float32(0.299)) * v[..., 0] + f(np.float32(0.587)) * v[..., 1]) + f(np.float32(0.114)) * v[..., 2]
        v = (f(1) - alpha) * v + alpha * L[..., None]
    return v.astype(f)


def augment(images, src_index, params, seed, H, W, dtype=np.float64):
    """the oracle of one call: images = the cache as a list of uint8 [h, w, 3] arrays; -> [N, H, W, 3] in [0, 1], not yet rounded to bf16"""
    params = np.asarray(params, dtype=np.float32)
    out = np.empty((len(src_index), H, W, 3), dtype=dtype)
    for n, s in enumerate(src_index):
        v = stages(images[s], params[n], seed, n, H, W, dtype)
        out[n] = np.clip(v, dtype(0), dtype(255)) / dtype(255)
    return out
