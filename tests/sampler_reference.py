"""A numpy restatement of the reference's four samplers (src/samplers/independent.cpp, pcg32.cpp, sobol.cpp, padded_sobol.cpp under
tile_shared.cpp, with src/util/rng.cpp): start, 1-D, 2-D and pixel-2-D draws for arrays of streams.  The arithmetic is integer except for the
final scale; the Sobol tables come from scene.view().sampler.  tests/test_sampler_reference.py pins it to oracle_sampler_stream bit for bit;
the GPU tests hold lrhip_query_sampler's mixed patterns to it, because the oracle's hook draws 1-D numbers only and PaddedSobol's 2-D draw
is not two of them."""
import ctypes as C

import numpy as np

INDEPENDENT, SOBOL, PADDED_SOBOL, PCG32 = 0, 1, 2, 3  # lr_scene.h: LR_SAMPLER_*
SOBOL_DIMENSIONS, SOBOL_MATRIX_SIZE = 1024, 52        # src/util/sobolmatrices.h:13-14
ONE_MINUS_EPSILON = np.float32(np.nextafter(np.float32(1), np.float32(0)))
P2, P3, P4, P5 = np.uint32(2246822519), np.uint32(3266489917), np.uint32(668265263), np.uint32(374761393)
U32 = np.uint32


def _u32(a):
    return np.asarray(a, dtype=np.uint32)


def _table(address, ctype, shape):
    # a copy of the table an lr_sampler points to (the view holds plain addresses)
    return np.ctypeslib.as_array(C.cast(address, C.POINTER(ctype)), shape=shape).copy()


def _rot17(h):
    return (h << U32(17)) | (h >> U32(15))


def _avalanche(h):
    h = P2 * (h ^ (h >> U32(15)))
    h = P3 * (h ^ (h >> U32(13)))
    return h ^ (h >> U32(16))


def xxhash32_1(p):  # rng.cpp:12-23
    with np.errstate(over="ignore"):
        return _avalanche(P4 * _rot17(_u32(p) + P5))


def xxhash32_2(x, y):  # rng.cpp:25-36
    with np.errstate(over="ignore"):
        return _avalanche(P4 * _rot17(_u32(y) + P5 + _u32(x) * P3))


def xxhash32_4(x, y, z, w):  # rng.cpp:53-69
    with np.errstate(over="ignore"):
        h = P4 * _rot17(_u32(w) + P5 + _u32(x) * P3)
        h = P4 * _rot17(h + _u32(y) * P3)
        h = P4 * _rot17(h + _u32(z) * P3)
        return _avalanche(h)


def unit_float(u):  # uniform_uint_to_float, rng.cpp:128-130
    return np.minimum(ONE_MINUS_EPSILON, _u32(u).astype(np.float32) * np.float32(2.0 ** -32))


def reverse_bits(v):
    v = _u32(v)
    v = ((v >> U32(1)) & U32(0x55555555)) | ((v & U32(0x55555555)) << U32(1))
    v = ((v >> U32(2)) & U32(0x33333333)) | ((v & U32(0x33333333)) << U32(2))
    v = ((v >> U32(4)) & U32(0x0F0F0F0F)) | ((v & U32(0x0F0F0F0F)) << U32(4))
    v = ((v >> U32(8)) & U32(0x00FF00FF)) | ((v & U32(0x00FF00FF)) << U32(8))
    return (v >> U32(16)) | (v << U32(16))


def owen_scramble(seed, v):  # _fast_owen_scramble, sobol.cpp:40-48
    seed = _u32(seed)
    with np.errstate(over="ignore"):
        v = reverse_bits(v)
        v = v ^ (v * U32(0x3D20ADEA))
        v = v + seed
        v = v * ((seed >> U32(16)) | U32(1))
        v = v ^ (v * U32(0x05526C56))
        v = v ^ (v * U32(0x53A22864))
        return reverse_bits(v)


def permutation_element(i, l, p):  # padded_sobol.cpp:59-91
    i, p = _u32(i).copy(), _u32(p)
    w = l - 1
    for s in (1, 2, 4, 8, 16):
        w |= w >> s
    w, l32 = U32(w), U32(l)
    todo = np.ones(i.shape, bool)
    with np.errstate(over="ignore"):
        while todo.any():
            k = i[todo]
            q = p[todo] if p.shape == i.shape else p
            k ^= q
            k *= U32(0xE170893D)
            k ^= q >> U32(16)
            k ^= (k & w) >> U32(4)
            k ^= q >> U32(8)
            k *= U32(0x0929EB3F)
            k ^= q >> U32(23)
            k ^= (k & w) >> U32(1)
            k *= U32(1) | (q >> U32(27))
            k *= U32(0x6935FA69)
            k ^= (k & w) >> U32(11)
            k *= U32(0x74DCB303)
            k ^= (k & w) >> U32(2)
            k *= U32(0x9E501CC3)
            k ^= (k & w) >> U32(2)
            k *= U32(0xC860A3DF)
            k &= w
            k ^= k >> U32(5)
            i[todo] = k
            todo[todo] = k >= l32
        return (i + p) % l32


class Samplers:
    """The sampler of scene.view() (an lr_sampler with its tables) for arrays of streams: start(px, py, index), then next_1d / next_2d /
    next_pixel_2d in any order.  Every draw returns float32."""

    def __init__(self, view):
        s = view.sampler
        self.kind, self.seed, self.spp, self.scale = int(s.kind), U32(s.seed), int(s.spp), int(s.scale)
        self.width, self.height = int(view.camera.width), int(view.camera.height)
        self.tile = (int(s.tile_size[0]), int(s.tile_size[1]))
        self.jitter = int(s.tile_jitter) != 0
        if self.kind in (SOBOL, PADDED_SOBOL):
            self.matrices = _table(s.sobol_matrices, C.c_uint32, (SOBOL_DIMENSIONS, SOBOL_MATRIX_SIZE))
        self.m = self.scale.bit_length() - 1
        if self.kind == SOBOL and self.m > 0:
            self.vdc = _table(s.vdc_sobol, C.c_uint64, (SOBOL_MATRIX_SIZE,))
            self.vdc_inv = _table(s.vdc_sobol_inv, C.c_uint64, (SOBOL_MATRIX_SIZE,))

    # ---- start
    def start(self, px, py, index):
        x, y = _u32(px).copy(), _u32(py).copy()
        index = np.broadcast_to(_u32(index), x.shape).copy()
        if self.tile[0] != 0:  # TileSharedSamplerInstance::start, tile_shared.cpp:51-62
            if self.jitter:
                offset = xxhash32_1(index)
                ox = (offset >> U32(16)).astype(np.float32) * np.float32(2.0 ** -16)
                oy = (offset & U32(0xFFFF)).astype(np.float32) * np.float32(2.0 ** -16)
                x = x + (ox * np.float32(self.width)).astype(np.uint32) % U32(self.width)
                y = y + (oy * np.float32(self.height)).astype(np.uint32) % U32(self.height)
            x, y = x // U32(self.tile[0]), y // U32(self.tile[1])
        self.x, self.y, self.index = x, y, index
        if self.kind == INDEPENDENT:  # independent.cpp:57-59
            self.state = xxhash32_4(x, y, self.seed, index)
        elif self.kind == PCG32:  # PCG32::set_sequence, rng.cpp:150-156
            self.state = np.zeros(x.shape, np.uint64)
            self.inc = (xxhash32_4(x, y, self.seed, index).astype(np.uint64) << np.uint64(1)) | np.uint64(1)
            self._pcg()
            with np.errstate(over="ignore"):
                self.state = self.state + np.uint64(0x853C49E6748FEA9B)
            self._pcg()
        elif self.kind == SOBOL:  # sobol.cpp:131-136, _sobol_interval_to_index :67-96
            self.dimension = np.full(x.shape, 2, np.uint32)
            frame = index.astype(np.uint64)
            if self.m == 0:
                self.sobol_index = frame
            else:
                idx = frame << np.uint64(2 * self.m)
                delta = np.zeros(x.shape, np.uint64)
                for c in range(32):
                    delta ^= np.where((frame >> np.uint64(c)) & np.uint64(1) != 0, self.vdc[c], np.uint64(0))
                b = delta ^ ((x.astype(np.uint64) << np.uint64(self.m)) | y.astype(np.uint64))
                for d in range(SOBOL_MATRIX_SIZE):
                    idx ^= np.where((b >> np.uint64(d)) & np.uint64(1) != 0, self.vdc_inv[d], np.uint64(0))
                assert (b >> np.uint64(SOBOL_MATRIX_SIZE) == 0).all()
                self.sobol_index = idx
        else:  # padded_sobol.cpp:113-117
            self.dimension = np.zeros(x.shape, np.uint32)

    def _pcg(self):  # PCG32::uniform_uint, rng.cpp:142-148
        old = self.state
        with np.errstate(over="ignore"):
            self.state = old * np.uint64(0x5851F42D4C957F2D) + self.inc
        xorshifted = (((old >> np.uint64(18)) ^ old) >> np.uint64(27)).astype(np.uint32)
        rot = (old >> np.uint64(59)).astype(np.uint32)
        with np.errstate(over="ignore"):
            return (xorshifted >> rot) | (xorshifted << ((~rot + U32(1)) & U32(31)))

    def _sobol_bits(self, a, dimension):  # _sobol_sample without its scramble and scale: sobol.cpp:52-60, padded_sobol.cpp:44-52
        a = np.asarray(a).astype(np.uint64)
        dimension = np.broadcast_to(_u32(dimension), a.shape)
        v = np.zeros(a.shape, np.uint32)
        for i in range(SOBOL_MATRIX_SIZE):
            v ^= np.where((a >> np.uint64(i)) & np.uint64(1) != 0, self.matrices[dimension, i], U32(0))
        assert (a >> np.uint64(SOBOL_MATRIX_SIZE) == 0).all()
        return v

    def _scaled(self, v):
        return _u32(v).astype(np.float32) * np.float32(2.0 ** -32)

    # ---- draws
    def next_1d(self):
        if self.kind == INDEPENDENT:  # lcg, rng.cpp:132-140
            with np.errstate(over="ignore"):
                self.state = U32(1664525) * self.state + U32(1013904223)
            return unit_float(self.state)
        if self.kind == PCG32:
            return unit_float(self._pcg())
        if self.kind == SOBOL:  # sobol.cpp:147-153
            self.dimension = np.where(self.dimension >= SOBOL_DIMENSIONS, U32(2), self.dimension)
            u = self._scaled(owen_scramble(xxhash32_2(self.dimension, self.seed), self._sobol_bits(self.sobol_index, self.dimension)))
            self.dimension = self.dimension + U32(1)
            return np.clip(u, np.float32(0), ONE_MINUS_EPSILON)
        h = xxhash32_4(self.x, self.y, self.index ^ self.seed, self.dimension)  # padded_sobol.cpp:128-137
        i = permutation_element(self.index, self.spp, h)
        self.dimension = self.dimension + U32(1)
        return np.minimum(self._scaled(owen_scramble(h, self._sobol_bits(i, 0))), ONE_MINUS_EPSILON)

    def next_2d(self):
        if self.kind == SOBOL:  # sobol.cpp:154-162
            self.dimension = np.where(self.dimension + U32(1) >= SOBOL_DIMENSIONS, U32(2), self.dimension)
            ux = self._scaled(owen_scramble(xxhash32_2(self.dimension, self.seed), self._sobol_bits(self.sobol_index, self.dimension)))
            uy = self._scaled(owen_scramble(xxhash32_2(self.dimension + U32(1), self.seed),
                                            self._sobol_bits(self.sobol_index, self.dimension + U32(1))))
            self.dimension = self.dimension + U32(2)
            return np.clip(np.stack([ux, uy], axis=-1), np.float32(0), ONE_MINUS_EPSILON)
        if self.kind == PADDED_SOBOL:  # padded_sobol.cpp:138-149: ONE permutation for both dimensions
            hx = xxhash32_4(self.x, self.y, self.index ^ self.seed, self.dimension)
            hy = xxhash32_4(self.x, self.y, self.index ^ self.seed, self.dimension + U32(1))
            i = permutation_element(self.index, self.spp, hx)
            self.dimension = self.dimension + U32(2)
            ux = np.minimum(self._scaled(owen_scramble(hx, self._sobol_bits(i, 0))), ONE_MINUS_EPSILON)
            uy = np.minimum(self._scaled(owen_scramble(hy, self._sobol_bits(i, 1))), ONE_MINUS_EPSILON)
            return np.stack([ux, uy], axis=-1)
        ux = self.next_1d()
        return np.stack([ux, self.next_1d()], axis=-1)

    def next_pixel_2d(self):  # sampler.h:48 (default: generate_2d); sobol.cpp:163-169
        if self.kind != SOBOL:
            return self.next_2d()
        s = np.float32(self.scale)
        ux = self._scaled(self._sobol_bits(self.sobol_index, 0)) * s - self.x.astype(np.float32)
        uy = self._scaled(self._sobol_bits(self.sobol_index, 1)) * s - self.y.astype(np.float32)
        return np.clip(np.stack([ux, uy], axis=-1), np.float32(0), ONE_MINUS_EPSILON)

    def draw(self, pattern: str):
        """the numbers of a sampler_draw pattern ("1", "2", "p"), [N, D]"""
        cols = []
        for c in pattern:
            u = {"1": self.next_1d, "2": self.next_2d, "p": self.next_pixel_2d}[c]()
            cols.extend([u] if c == "1" else [u[..., 0], u[..., 1]])
        n = self.x.shape[0]
        return np.stack(cols, axis=-1).astype(np.float32) if cols else np.zeros((n, 0), np.float32)


def oracle_stream(oracle_lib, view, px, py, index, n):
    """oracle_sampler_stream: the pixel pair and n following 1-D draws of one stream, float32 [2 + n]"""
    out = np.zeros(2 + n, np.float32)
    oracle_lib.oracle_sampler_stream(C.byref(view), int(px), int(py), int(index), int(n), out.ctypes.data)
    return out


def scene_text(sampler: str, tile=None, jitter=False, **kwargs) -> str:
    """the 64 x 64 Cornell box with the named sampler, optionally under TileShared"""
    from luisarender_amd.scenes import cornell_box
    kwargs.setdefault("resolution", 64)
    kwargs.setdefault("spp", 8)
    text = cornell_box(sampler=sampler, **kwargs)
    if tile is not None:
        seed = kwargs.get("seed", 19980810)
        inner = f"sampler : {sampler} {{ seed {{ {seed} }} }}"
        assert inner in text
        text = text.replace(inner, f"sampler : TileShared {{ tile_size {{ {tile} }} jitter {{ {'true' if jitter else 'false'} }} "
                                   f"base : {sampler} {{ seed {{ {seed} }} }} }}")
    return text


SAMPLER_CASES = [("Independent", None, False), ("PCG32", None, False), ("Sobol", None, False), ("PaddedSobol", None, False),
                 ("Independent", 8, False), ("PaddedSobol", 8, True), ("Sobol", 16, True), ("PCG32", 4, False)]
