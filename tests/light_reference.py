"""Reference of the light queries (include/lrhip.h: lrhip_query_light): the reference's light sampling restated in float64 numpy
from the HOST tables of a Scene -- UniformLightSampler::select, _sample_area and _sample_environment for a constant environment
(src/lightsamplers/uniform.cpp:78-143), with the alias pick (src/util/sampling.h:38-66), sample_uniform_triangle and sample_uniform_sphere
(src/util/sampling.cpp:89-108), DiffuseLight's evaluation (src/lights/diffuse.cpp:67-88) and spawn_ray_to's 0.9999 (src/base/interaction.cpp:25-30).

Everything is widened to float64 FIRST: the float32 tables, the float32 random numbers, the float32 points.  The one float32 piece is the ray
origin, Interaction::p_robust (interaction.cpp:13-19) with LuisaCompute's offset_ray_origin, which works on the bits of float32 numbers.
What the device disagrees with this about is its float32 arithmetic (or its code).

Also here: the scenes of tests/test_gpu_light.py, their inputs, and the errors measured on the MI355X that its bars are made of."""
import ctypes as C
import functools

import numpy as np

import surface_reference as R
from instance_scene import _words, host_tables
from luisarender_amd import Scene

INVALID = 0xFFFFFFFF
COUNT = 4 * 256 + 3  # more than one block of 256 lanes, and not a multiple of it
KIND_AREA, KIND_ENVIRONMENT, KIND_NONE = 0, 1, 2  # lrhip.h: LRHIP_LIGHT_KIND_*
FLT_MAX = float(np.finfo(np.float32).max)
SHADOW_SCALE = float(np.float32(0.9999))

# The largest errors of the device against this reference / the closed forms, measured on the MI355X over COUNT records per scene
# (tests/test_gpu_light.py prints them): pdf and L componentwise |dev - ref| / max(|ref|, 1e-2), the ray's origin and direction componentwise
# absolute (the scenes are of unit scale), t_max relative.  The bars are MARGIN x the recorded values, the project's margin for a
# float32-against-float64 bar; a measured error above bsdf_reference.LARGEST_SOUND_ERROR would be a bug to find, not a bar to
# set.  (None would mean: not measured yet -- the test then fails after printing its figures.)  No record of any case flipped.
MEASURED_CLOSED_FORM_PDF = 1.60e-5  # case 1: pdf against dist^2 / (|cos| A) / 2 from the returned point
MEASURED_REFERENCE_PDF = 8.20e-7    # case 2: against sample() below
MEASURED_REFERENCE_L = 2.49e-8          # (the constant environment's L: the float32 product of colour and scale)
MEASURED_REFERENCE_ORIGIN = 4.77e-7     # (two ulp of a coordinate between 2 and 4)
MEASURED_REFERENCE_DIRECTION = 2.97e-7
MEASURED_REFERENCE_T_MAX = 3.05e-7
MEASURED_EVALUATE_PDF = 3.79e-5     # case 3: light_evaluate at the traced shadow ray's hit against the sample, the largest over the scenes
MEASURED_EVALUATE_L = 1.89e-5           # (the image environment: the texture lookup at the direction's uv against the sampled uv; 0.0 for constant emission)
MEASURED_POINTS = 5.73e-6           # case 5: points mode against hits mode in L, pdf and d
MEASURED_PATHS_P = 3.96e-7          # case 7: the sampled point of the baked path against the instance path's, on the moved scene
MARGIN = 4.0
MAX_FLIPS = 2          # records on which device and reference may disagree about the picked triangle or about environment against light
BOUNDARY = 1e-5        # the inputs stand this far from every table boundary, so that the reference alone gives no flip
# how far o + d t_max / 0.9999 may lie from its emitter's plane: the point is put together again from the float32 o, d and t_max, each good to
# half an ulp, over distances below 6 -- 16 x 2^-24 x 6, a bar from the number format (the tests print what they see)
PLANE_BAR = 16.0 * 2.0 ** -24 * 6.0
GRAZING = 1e-3         # a record is left out of the pdf comparison where the emitter is seen at |cos| below this


def _unit(a):
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


# ---------------------------------------------------------------- the host tables

def light_tables(scene: Scene) -> dict:
    """host_tables(scene) and what the light sampler reads beside them: tri_alias (prob float32, alias uint32) and tri_pdf [triangles],
    light_instances [n, 2] (instance_id, light_tag), per light node its constant L [3] and two_sided, env_prob, light_count, and for a constant
    Spherical environment its L [3] and env_to_world [3, 3] (row r, column c)"""
    v = scene.view()
    t = host_tables(scene)
    n = int(v.triangle_count)
    alias = _words(v.tri_alias, n, 8)
    t["alias_prob"], t["alias_index"] = alias[:, 0].view(np.float32).astype(np.float64), alias[:, 1].astype(np.int64)
    t["tri_pdf"] = np.frombuffer(C.string_at(v.tri_pdf, n * 4), np.float32).astype(np.float64) if n else np.zeros(0)
    t["light_instances"] = _words(v.light_instances, v.light_instance_count, 8).astype(np.int64)

    def constant(tex, scale):
        ch = [float(x) for x in tex.v]
        rgb = np.array(ch[0:1] * 3 if tex.channels == 1 else ch[0:3])
        return np.maximum(rgb, 0.0) * float(scale)  # evaluate_illuminant_spectrum of a Constant texture, clamped, times the node's scale

    t["light_L"] = np.array([constant(v.textures[v.lights[i].emission_tex], v.lights[i].scale) for i in range(v.light_count)]).reshape(-1, 3)
    t["light_two_sided"] = np.array([v.lights[i].two_sided != 0 for i in range(v.light_count)], bool)
    t["env_prob"], t["light_count"] = float(v.integrator.env_prob), int(v.integrator.light_count)
    env = v.environment
    if env.kind != 0 and env.emission_tex >= 0:
        t["env_L"] = constant(v.textures[env.emission_tex], env.scale)
        t["env_to_world"] = np.array([float(x) for x in env.env_to_world]).reshape(3, 3).T  # stored column-major
    return t


# ---------------------------------------------------------------- the reference's pieces

def select(env_prob: float, light_count: int, u):
    """UniformLightSampler::select, uniform.cpp:78-90 -> (is_env bool [N], tag int [N], prob [N])"""
    u = np.asarray(u, np.float64)
    n = float(light_count)
    if env_prob == 1.0:
        return np.ones(u.shape, bool), np.zeros(u.shape, np.int64), np.ones(u.shape)
    if env_prob == 0.0:
        return np.zeros(u.shape, bool), np.clip(u * n, 0.0, n - 1.0).astype(np.int64), np.full(u.shape, 1.0 / n)
    uu = (u - env_prob) / (1.0 - env_prob)
    is_env = u < env_prob
    tag = np.clip(uu * n, 0.0, n - 1.0).astype(np.int64)
    return is_env, np.where(is_env, 0, tag), np.where(is_env, env_prob, (1.0 - env_prob) / n)


def alias_pick(prob, index, u):
    """sample_alias_table, sampling.h:38-66, over ONE table (prob, index [n]) -> (picked entry int [N], the remapped u [N])"""
    u = np.asarray(u, np.float64)
    n = len(prob)
    x = u * n
    slot = np.clip(x.astype(np.int64), 0, n - 1)
    ur = x - np.floor(x)
    p = prob[slot]
    stay = ur < p
    with np.errstate(all="ignore"):
        return np.where(stay, slot, index[slot]), np.where(stay, ur / p, (ur - p) / (1.0 - p))


def alias_boundary_distance(prob, u):
    """how far (in u) each u stands from the nearest decision boundary of alias_pick over the table: a slot edge k / n or a slot's
    (k + prob[k]) / n"""
    u = np.asarray(u, np.float64)
    n = len(prob)
    edges = np.concatenate([np.arange(n + 1) / n, (np.arange(n) + prob) / n])
    return np.abs(u[:, None] - edges[None, :]).min(axis=1)


def sample_uniform_triangle(ux, uy):
    """sampling.cpp:89-98 -> barycentric weights [N, 3] of the triangle's vertices 0, 1, 2"""
    ux, uy = np.asarray(ux, np.float64), np.asarray(uy, np.float64)
    a = np.where(ux < uy, 0.5 * ux, -0.5 * uy + ux)
    b = np.where(ux < uy, -0.5 * ux + uy, 0.5 * uy)
    return np.stack([a, b, 1.0 - a - b], axis=1)


def sample_uniform_sphere(ux, uy):
    """sampling.cpp:100-108"""
    z = 1.0 - 2.0 * np.asarray(ux, np.float64)
    r = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    phi = 2.0 * np.pi * np.asarray(uy, np.float64)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def offset_ray_origin(p, n):
    """LuisaCompute's offset_ray_origin (Ray Tracing Gems ch. 6) in float32, componentwise on [N, 3] arrays"""
    p, n = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(n, np.float32)
    of_i = (np.float32(256.0) * n).astype(np.int32)  # truncation, as the reference's cast
    p_i = (p.view(np.int32) + np.where(p < 0, -of_i, of_i)).view(np.float32)
    return np.where(np.abs(p) < np.float32(1.0 / 32.0), p + np.float32(1.0 / 65536.0) * n, p_i)


def robust_origin(p, ng, ns, offset_bits, w):
    """Interaction::p_robust(w), interaction.cpp:13-19: p moved off its surface to the side of ng that w points to (judged by ns), by the
    shape's intersection-offset factor (shape.cpp:88-93).  offset_bits None: Interaction{p} of a medium point, p itself."""
    p = np.asarray(p, np.float32)
    if offset_bits is None:
        return p.astype(np.float64)
    x = (np.asarray(offset_bits, np.int64) & 0xFFFF).astype(np.float32) * np.float32(1.0 / 65536.0)
    factor = np.clip(x * np.float32(255.0) + np.float32(1.0), np.float32(1.0), np.float32(256.0))
    front = np.einsum("nk,nk->n", np.asarray(ns, np.float64), np.asarray(w, np.float64)) > 0.0
    n = np.where(front[:, None], ng, -np.asarray(ng)).astype(np.float32)
    return offset_ray_origin(p, factor[:, None] * n).astype(np.float64)


def evaluate_area(t: dict, inst, prim, lp: dict, p_from):
    """DiffuseLightClosure::_evaluate, diffuse.cpp:67-88, for the light points lp = surface_reference.shading_points(...) of (inst, prim)
    seen from p_from [N, 3] -> (L [N, 3], pdf [N]) WITHOUT the selection probability; back_facing by dot(ng, p_from - p) < 0"""
    inst, prim = np.asarray(inst, np.int64), np.asarray(prim, np.int64)
    rec = t["instances"][inst]
    tag = (rec[:, 1] & 4095).astype(np.int64)
    tri_offset = t["meshes"][rec[:, 0] >> 10][:, 2].astype(np.int64)
    pdf_area = t["tri_pdf"][tri_offset + prim] / lp["area"]
    to_from = np.asarray(p_from, np.float64) - lp["p"]
    with np.errstate(all="ignore"):
        cos_wo = np.abs(np.einsum("nk,nk->n", _unit(to_from), lp["ng"]))
        pdf = np.einsum("nk,nk->n", to_from, to_from) * pdf_area / cos_wo
    back = np.einsum("nk,nk->n", lp["ng"], to_from) < 0.0
    invalid = ~(cos_wo >= 1e-6) | (~t["light_two_sided"][tag] & back)
    return np.where(invalid[:, None], 0.0, t["light_L"][tag]), np.where(invalid, 0.0, pdf)


def sample(t: dict, p, ng, ns, offset_bits, u) -> dict:
    """LightSampler::Instance::sample (light_sampler.cpp:57-63) at the points p [N, 3] with normals ng, ns and handle.w offset_bits [N] (None:
    bare points) for the random numbers u [N, 3] -> dict over the N records: kind, L [N, 3], pdf (times the selection probability), the
    shadow ray o, d [N, 3], t_max, and for area samples inst, prim (the picked triangle) and point [N, 3] (the sampled light point)"""
    p, u = np.asarray(p, np.float32).astype(np.float64), np.asarray(u, np.float32).astype(np.float64)
    n = len(p)
    is_env, tag, prob = select(t["env_prob"], t["light_count"], u[:, 0])
    out = {"kind": np.where(is_env, KIND_ENVIRONMENT, KIND_AREA), "L": np.zeros((n, 3)), "pdf": np.zeros(n), "o": np.zeros((n, 3)),
           "d": np.zeros((n, 3)), "t_max": np.zeros(n), "inst": np.full(n, -1, np.int64), "prim": np.full(n, -1, np.int64), "point": np.zeros((n, 3))}
    sub = lambda a, m: None if a is None else np.asarray(a)[m]  # noqa: E731
    if is_env.any():  # _sample_environment of a constant Spherical, spherical.cpp:114-118,138
        m = is_env
        wi = _unit(sample_uniform_sphere(u[m, 1], u[m, 2]) @ t["env_to_world"].T)
        out["L"][m], out["pdf"][m] = t["env_L"], prob[m] / (4.0 * np.pi)
        out["o"][m], out["d"][m], out["t_max"][m] = robust_origin(p[m], sub(ng, m), sub(ns, m), sub(offset_bits, m), wi), wi, FLT_MAX
    if (~is_env).any():  # _sample_area, uniform.cpp:107-123
        m = ~is_env
        inst = t["light_instances"][tag[m], 0]
        mesh = t["meshes"][t["instances"][inst, 0] >> 10]
        prim, ux = np.zeros(m.sum(), np.int64), np.zeros(m.sum())
        for i in np.unique(inst):  # one alias table per emitting mesh
            k = inst == i
            first, count = int(mesh[k][0, 2]), int(mesh[k][0, 3])
            prim[k], ux[k] = alias_pick(t["alias_prob"][first:first + count], t["alias_index"][first:first + count], u[m, 1][k])
        w = sample_uniform_triangle(ux, u[m, 2])
        lp = R.shading_points(t, inst, prim, w[:, 1], w[:, 2])
        L, pdf = evaluate_area(t, inst, prim, lp, p[m])
        o = robust_origin(p[m], sub(ng, m), sub(ns, m), sub(offset_bits, m), lp["p"] - p[m])  # spawn_ray_to, interaction.cpp:25-30
        to_light = lp["p"] - o
        dist = np.linalg.norm(to_light, axis=1)
        out["L"][m], out["pdf"][m] = L, pdf * prob[m]
        out["o"][m], out["d"][m], out["t_max"][m] = o, to_light / dist[:, None], dist * SHADOW_SCALE
        out["inst"][m], out["prim"][m], out["point"][m] = inst, prim, lp["p"]
    return out


def relative_error(dev, ref) -> np.ndarray:
    """componentwise |dev - ref| / max(|ref|, 1e-2), in float64"""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    return np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-2)


def invalid_result() -> np.ndarray:
    """the invalid record's result as 8 words: zeros, except kind = LR_INVALID_ID"""
    r = np.zeros(8, np.uint32)
    r[4] = INVALID
    return r


# ---------------------------------------------------------------- the scenes of tests/test_gpu_light.py

# case 1: a matte floor, a two-sided emitter of area A = 1.5 x 1 above it and a one-sided one of another colour that faces AWAY from
# the part of the floor with x < -1 (its plane is x = -1, its normal +x), no environment
PANEL_A = {"corner": np.array([-0.25, 2.0, -0.5]), "e1": np.array([1.5, 0.0, 0.0]), "e2": np.array([0.0, 0.0, 1.0]), "L": np.float32([6.0, 5.0, 4.0])}
PANEL_B = {"corner": np.array([-1.0, 0.5, -0.5]), "e1": np.array([0.0, 0.0, 1.0]), "e2": np.array([0.0, 1.0, 0.0]), "L": np.float32([1.0, 2.0, 3.0])}
TWO_PANELS = """
Shape floor : InlineMesh { positions { -3,0,-3, 3,0,-3, 3,0,3, -3,0,3 } indices { 0,2,1, 0,3,2 } surface : Matte { Kd : Constant { v { 0.6 } } } }
Shape panel_a : InlineMesh { positions { -0.25,2,-0.5, 1.25,2,-0.5, 1.25,2,0.5, -0.25,2,0.5 } indices { 0,1,2, 0,2,3 }
  light : Diffuse { emission : Constant { v { 6, 5, 4 } } two_sided { true } } }
Shape panel_b : InlineMesh { positions { -1,0.5,-0.5, -1,0.5,0.5, -1,1.5,0.5, -1,1.5,-0.5 } indices { 0,2,1, 0,3,2 }
  light : Diffuse { emission : Constant { v { 1, 2, 3 } } two_sided { false } } }
Camera cam : Pinhole { film : Color { resolution { 8, 8 } } spp { 1 } position { 0, 1, 6 } look_at { 0, 1, 0 } }
render { cameras { @cam } shapes { @floor, @panel_a, @panel_b } integrator : MegaPath { } }
"""

# case 2: a five-triangle fan of unequal triangles (areas 0.1 .. 0.8: no trivial alias table) as the emitter, a second, plain emitter, and a
# constant environment with 0 < env_prob < 1
FAN = """
Shape floor : InlineMesh { positions { -3,0,-3, 3,0,-3, 3,0,3, -3,0,3 } indices { 0,2,1, 0,3,2 } surface : Matte { Kd : Constant { v { 0.6 } } } }
Shape fan : InlineMesh { positions { 0,2,0, 1,2,0, 0.9,2,0.2, 0.6,2,0.9, -0.5,2,1.1, -1.2,2,-0.3, -0.2,2,-1.6 } indices { 0,2,1, 0,3,2, 0,4,3, 0,5,4, 0,6,5 }
  light : Diffuse { emission : Constant { v { 4, 3, 2 } } two_sided { true } } transform : SRT { rotate { 1, 0, 0.3, 25 } translate { 0.2, 0.3, -0.1 } } }
Shape lamp : InlineMesh { positions { -2,1,-2, -1.5,1,-2, -1.5,1.5,-2, -2,1.5,-2 } indices { 0,1,2, 0,2,3 }
  light : Diffuse { emission : Constant { v { 9, 9, 1 } } two_sided { true } } }
Camera cam : Pinhole { film : Color { resolution { 8, 8 } } spp { 1 } position { 0, 1, 6 } look_at { 0, 1, 0 } }
render { cameras { @cam } shapes { @floor, @fan, @lamp } environment : ENV integrator : MegaPath { } }
"""
FAN_CONSTANT = "Spherical { emission : Constant { v { 0.3, 0.5, 0.8 } } scale { 1.5 } transform : SRT { rotate { 0.3, 1, 0.2, 70 } } }"


def fan_scene(env: str = FAN_CONSTANT) -> str:
    return FAN.replace("ENV", env)


@functools.lru_cache(maxsize=None)
def inputs(seed: int = 31) -> dict:
    """COUNT records shared by the cases, float32: floor points (x, z uniform in [-2.5, 2.5]^2, y = 0) as rays that look straight down at
    them from y = 1, and u [N, 3] uniform in [0, 1)"""
    rng = np.random.default_rng(seed)
    xz = rng.uniform(-2.5, 2.5, (COUNT, 2))
    rays = np.zeros((COUNT, 8), np.float32)
    rays[:, 0], rays[:, 1], rays[:, 2] = xz[:, 0], 1.0, xz[:, 1]
    rays[:, 5], rays[:, 7] = -1.0, np.inf
    u = np.minimum(rng.random((COUNT, 3)).astype(np.float32), np.nextafter(np.float32(1.0), np.float32(0.0)))
    for a in (rays, u):
        a.setflags(write=False)
    return {"rays": rays, "u": u, "p": np.stack([rays[:, 0], np.zeros(COUNT, np.float32), rays[:, 2]], axis=1)}


def floor_frame(n: int) -> tuple:
    """ng, ns of the floors above (winding 0,2,1 / 0,3,2 of a y = 0 quad: +y) for n records"""
    up = np.tile(np.array([0.0, 1.0, 0.0]), (n, 1))
    return up, up


def panel_of(point, panel, tolerance):
    """(distance of each point [N, 3] from the panel's plane, whether it lies inside the panel's rectangle to the tolerance)"""
    e1, e2 = panel["e1"], panel["e2"]
    normal = _unit(np.cross(e1, e2))
    rel = np.asarray(point, np.float64) - panel["corner"]
    a, b = rel @ e1 / (e1 @ e1), rel @ e2 / (e2 @ e2)
    inside = (a >= -tolerance) & (a <= 1.0 + tolerance) & (b >= -tolerance) & (b <= 1.0 + tolerance)
    return np.abs(rel @ normal), inside
