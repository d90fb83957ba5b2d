"""The edge-avoiding a-trous wavelet filter of DESIGN §4.8 restated in numpy, and the synthetic frames the denoiser's tests share
(tests/test_denoise.py on the CPU, tests/test_gpu_denoise.py against the device).  Nothing here calls the library."""
import functools

import numpy as np

KERNEL = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
# lrhip.h's LRHIP_DENOISE_DEFAULT_* (test_denoise.py compares), and the parameters of the synthetic cases: the values the dropped-tap and
# wrong-step figures below were measured with -- they stay whatever the defaults become
DEFAULTS = {"iterations": 5, "sigma_color": 0.9, "sigma_normal": 0.35, "sigma_depth": 0.1, "demodulate": True}
SYNTHETIC_PARAMS = {"iterations": 5, "sigma_color": 4.0, "sigma_normal": 0.35, "sigma_depth": 0.1, "demodulate": True}
SIZES = ((23, 37), (45, 70), (7, 9), (1, 1))  # (height, width); at 7 x 9 every tap of the later passes falls outside the image

# Largest |device - float64 restatement| / (|restatement| + 1e-6) over pixels and channels that the device may show on the synthetic
# frames: 4 x the value measured on the MI355X (headroom for the hardware exponential and fma contraction, which vary with the compiler).
# It may never exceed 1e-4: dropping ONE tap of pass 0 moves these frames by more than twice that (test_denoise.py asserts it).
MEASURED_DEVICE_ERROR = 8.0e-7  # 4.7e-7 at 23 x 37, 7.9e-7 at 45 x 70, 2.6e-7 at 7 x 9, 0 at 1 x 1
DEVICE_BAR = 4 * MEASURED_DEVICE_ERROR
assert DEVICE_BAR <= 1e-4


def atrous(color, albedo, normal, depth, iterations=5, sigma_color=4.0, sigma_normal=0.35, sigma_depth=0.1, demodulate=True,
           dtype=np.float64, drop_tap=None, steps=None):
    """color, albedo, normal [H, W, 3], depth [H, W] -> [H, W, 3], every operation in `dtype`.  drop_tap = (pass, dy, dx) leaves one tap
    out and steps = a list of step sizes replaces 2^i: the two mistakes the tests measure the filter's sensitivity with."""
    t = dtype
    c, a, n, z = (np.asarray(x).astype(t) for x in (color, albedo, normal, depth))
    z = z.reshape(z.shape[0], z.shape[1])
    ap = np.where(a > t(1e-3), a, t(1)) if demodulate else np.ones_like(a)
    u = c / ap
    h, w = z.shape
    for i in range(iterations):
        s = (1 << i) if steps is None else steps[i]
        sigma_i = t(sigma_color) * t(2.0 ** -i)
        r = (u[..., 0] + u[..., 1] + u[..., 2]) / t(3) + t(1e-4)
        scale_c = (sigma_i * r) ** 2
        scale_n = t(sigma_normal) ** 2
        scale_z = (t(sigma_depth) * (np.abs(z) + t(1e-4))) ** 2
        num, den = np.zeros_like(u), np.zeros((h, w), t)
        for dy in range(-2, 3):  # row-major order of (dy, dx)
            for dx in range(-2, 3):
                if drop_tap == (i, dy, dx):
                    continue
                y0, y1 = max(0, -dy * s), min(h, h - dy * s)
                x0, x1 = max(0, -dx * s), min(w, w - dx * s)
                if y0 >= y1 or x0 >= x1:  # every such tap is outside the image
                    continue
                p = (slice(y0, y1), slice(x0, x1))
                q = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                d = (((u[p] - u[q]) ** 2).sum(-1) / scale_c[p] + ((n[p] - n[q]) ** 2).sum(-1) / scale_n
                     + (z[p] - z[q]) ** 2 / scale_z[p])
                weight = t(KERNEL[dx + 2] * KERNEL[dy + 2]) * np.exp(-d).astype(t)
                num[p] += weight[..., None] * u[q]
                den[p] += weight
        u = num / den[..., None]
    return u * ap


@functools.lru_cache(maxsize=None)
def synthetic(height, width, seed=1):
    """A floor plane (its normal, a depth ramp, grey albedo), a back wall, a shaded ball (varying normals) and a sky strip (all guides
    zero); the colour is the clean shading times seeded gamma noise.  Returns read-only (noisy, albedo, normal, depth, clean)."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float32)
    normal = np.zeros((height, width, 3), np.float32)
    depth = np.zeros((height, width), np.float32)
    albedo = np.zeros((height, width, 3), np.float32)
    floor = yy > 0.6 * height
    wall = (yy <= 0.6 * height) & (yy > 0.15 * height)
    normal[floor], depth[floor], albedo[floor] = (0, 1, 0), 2 + 6 * (height - yy[floor]) / height, (0.7, 0.7, 0.7)
    normal[wall], depth[wall], albedo[wall] = (0, 0, 1), 8, (0.6, 0.2, 0.2)
    cx, cy, radius = 0.5 * width, 0.55 * height, 0.2 * min(height, width)
    ball = (xx - cx) ** 2 + (yy - cy) ** 2 < radius * radius
    nx, ny = (xx - cx) / max(radius, 1e-6), -(yy - cy) / max(radius, 1e-6)
    nz = np.sqrt(np.clip(1 - nx * nx - ny * ny, 0, 1))
    normal[ball], depth[ball], albedo[ball] = np.stack([nx, ny, nz], -1)[ball], (5 - nz)[ball], (0.2, 0.5, 0.8)
    sky = ~(floor | wall | ball)
    clean = albedo * (0.3 + 0.7 * np.clip(normal[..., 1:2] * 0.6 + normal[..., 2:3] * 0.5, 0, 1))
    clean[sky] = (0.5, 0.7, 1.0)
    noisy = clean * g.gamma(4.0, 0.25, (height, width, 1)).astype(np.float32) * g.uniform(0.8, 1.2, (height, width, 3)).astype(np.float32)
    noisy[sky] = (0.5, 0.7, 1.0)
    out = tuple(np.ascontiguousarray(x, np.float32) for x in (noisy, albedo, normal, depth, clean))
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def synthetic_reference(height, width):
    """atrous of synthetic(height, width) under SYNTHETIC_PARAMS, in float64; computed once, read-only"""
    noisy, albedo, normal, depth, _ = synthetic(height, width)
    ref = atrous(noisy, albedo, normal, depth, **SYNTHETIC_PARAMS)
    ref.setflags(write=False)
    return ref


def relative_error(got, ref):
    """the tests' metric: the largest |got - ref| / (|ref| + 1e-6) over pixels and channels"""
    return float((np.abs(np.asarray(got, np.float64) - ref) / (np.abs(ref) + 1e-6)).max())


def edge_case(height=12, width=16, seed=3):
    """Two half-images with orthogonal normals (side A: columns left of the middle) under noisy colours; equal depth and albedo"""
    g = np.random.default_rng(seed)
    normal = np.zeros((height, width, 3), np.float32)
    normal[:, : width // 2], normal[:, width // 2:] = (0, 1, 0), (1, 0, 0)
    color = g.uniform(0.2, 1.5, (height, width, 3)).astype(np.float32)
    other = color.copy()
    other[:, width // 2:] = g.uniform(2.0, 9.0, (height, width - width // 2, 3)).astype(np.float32)
    albedo = np.full((height, width, 3), 0.5, np.float32)
    depth = np.full((height, width), 3.0, np.float32)
    return color, other, albedo, normal, depth


def ulp_distance(a, b):
    """float32 arrays: how many representable floats apart (same sign assumed)"""
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))
