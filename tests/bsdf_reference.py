"""Reference of the BSDF queries (include/lrhip.h: lrhip_query_bsdf): the inputs the device is asked about, the oracle's answers
for them (oracle_surface_evaluate / oracle_surface_sample through tests/helpers.SurfaceProbe: Surface::Closure::evaluate / sample on a flat
patch with ng = ns = +z and the identity frame), and the rule that says which records the value comparison leaves out.

The device side of the comparison is tests/helpers.MATERIALS on a two-triangle quad in the z = 0 plane without uvs (QUAD below): its winding
gives ng = +z, and without uvs the device takes the fallback frame frame_from_normal(+z), the identity -- the oracle's flat_patch frame, so
SurfaceProbe's local directions ARE the world directions."""
import functools

import numpy as np

from helpers import MATERIALS, SurfaceProbe, material_scene

INVALID = 0xFFFFFFFF
COUNT = 4 * 256 + 3  # more than one block of 256 lanes, and not a multiple of it
SEED = 20

TRANSMISSIVE = ("glass", "disney_trans", "mix_glass")            # wo comes from below half the time (tests/test_oracle_bsdf.py)
LAYERED = ("layered", "layered_medium")                          # evaluate() is itself a random-walk estimator: compared by their means
NESTED = ("mix_layered", "layered_mix", "layered_layered")       # Mix / Layered in each other: lrhip_query_bsdf refuses the scene
DETERMINISTIC = tuple(m for m in MATERIALS if m not in LAYERED and m not in NESTED)
# sample() agrees with evaluate() at the sampled direction for these; the inner Mix nodes of the two trees take the reference's "sample b"
# quirk branch for some lobe numbers (tests/test_oracle_bsdf.py leaves them out for the same reason and pins the quirk on its own)
SELF_CONSISTENT = tuple(m for m in DETERMINISTIC if m not in ("mix_nested", "mix_deep"))
# the ratio of each Mix material's ROOT node: a lobe number at or above it takes the root's "sample b" branch (mix.cpp:186-193: the direction
# is drawn from child a with the remapped lobe number, child b is evaluated there, and the two are mixed with the roles swapped)
MIX_ROOT_RATIO = {"mix": 0.3, "mix_glass": 0.6, "mix_nested": 0.6, "mix_deep": 0.8}
CLASS_OF = {m: ("mix" if m.startswith("mix") else "disney" if m.startswith("disney") else "basic") for m in DETERMINISTIC}

QUAD = """
{surface}
Shape quad : InlineMesh {{ positions {{ -1,-1,0, 1,-1,0, 1,1,0, -1,1,0 }} indices {{ 0,1,2, 0,2,3 }} surface {{ @m }} }}
Camera cam : Pinhole {{ film : Color {{ resolution {{ 8, 8 }} }} spp {{ 1 }} position {{ 0, 0, 3 }} look_at {{ 0, 0, 0 }} }}
render {{ cameras {{ @cam }} shapes {{ @quad }} environment : Spherical {{ emission : Constant {{ v {{ 1 }} }} }} integrator : MegaPath {{ }} }}
"""

# The largest errors of the device against the oracle, measured on the MI355X over COUNT records per material, per class of material
# (tests/test_gpu_bsdf.py prints them): f and pdf componentwise |dev - ref| / max(|ref|, 1e-2), the sampled wi componentwise absolute, over the
# records that are not excluded and on which both agree that pdf > 0.  The bars are 4 x the recorded values, the project's margin for a
# float-against-float bar.  A measured error above 2e-3 -- what tests/test_oracle_bsdf.py allows between the oracle's own
# sample() and evaluate() -- would be a bug to find, not a bar to set.  The query's kernels are built with the oracle's arithmetic (no
# contraction, correctly rounded division and square root), so 0.0 is a measurement: on every such record the device's bits
# are the oracle's, and its bar asks for that.  What remains is the device's own sine and cosine (sample mode: the cosine-hemisphere and the
# near-normal GGX branch), exp of Plastic's absorption and the Disney lobes' powers.  No record of any material flipped (MAX_FLIPS allows 2).
# The first build, with the renderers' approximate division and square root, measured 43 flips on Glass (pdf 1e-8 for the oracle's 0 under
# total internal reflection) and sample-mode errors up to 5.9e-2 in f and pdf and 2.3e-3 in wi: above LARGEST_SOUND_ERROR, hence the flags.
MEASURED_EVALUATE_F = {"basic": 1.91e-7, "disney": 1.49e-6, "mix": 0.0}      # basic: plastic; every other basic closure 0.0
MEASURED_EVALUATE_PDF = {"basic": 0.0, "disney": 2.34e-6, "mix": 0.0}
MEASURED_SAMPLE_F = {"basic": 1.25e-5, "disney": 4.10e-5, "mix": 4.10e-6}    # basic: oren; disney: disney
MEASURED_SAMPLE_PDF = {"basic": 2.45e-5, "disney": 5.00e-5, "mix": 5.59e-6}  # basic: plastic
MEASURED_SAMPLE_WI = {"basic": 9.06e-7, "disney": 5.37e-7, "mix": 5.97e-7}
# The same for the Mix materials with u_lobe confined to the root's "sample b" branch (sample_b_inputs; test_gpu_bsdf.py:
# test_mix_sample_b_against_the_oracle), the largest over the four materials: measured, printed and barred in the same way
MEASURED_SAMPLE_B_F = 8.20e-6      # mix (Matte's direction, the Mirror evaluated there); mix_glass 1.9e-6, mix_nested 1.9e-6, mix_deep 5.2e-7
MEASURED_SAMPLE_B_PDF = 9.26e-6    # mix; mix_glass 1.8e-6, mix_nested 2.0e-6, mix_deep 2.1e-7
MEASURED_SAMPLE_B_WI = 5.96e-7     # mix; the others 1.2e-7 and less
LARGEST_SOUND_ERROR = 2e-3
MARGIN = 4.0
GRAZING = 1e-3        # a record is left out of the value comparison where |cos| of one of its directions is below this
MAX_FLIPS = 2         # records per material and mode on which device and oracle may disagree about pdf > 0 or the event


def scene_text(name: str) -> str:
    return QUAD.format(surface=MATERIALS[name])


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """the COUNT records of material `name`, float32: wo [N, 3] (theta in [0.05, 1.45], from below half the time for the transmissive
    materials), wi [N, 3] uniform on the sphere, u [N, 3] uniform in [0, 1) -- for the Mix materials u_lobe is confined to the "sample a"
    branch as in tests/test_oracle_bsdf.py --, and the point of the quad the record stands on: prim, (u, v) inside the triangle"""
    rng = np.random.default_rng([SEED, list(MATERIALS).index(name)])
    n = COUNT
    theta, phi = rng.uniform(0.05, 1.45, n), rng.uniform(0.0, 2.0 * np.pi, n)
    wo = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1).astype(np.float32)
    if name in TRANSMISSIVE:
        wo[rng.random(n) < 0.5, 2] *= -1.0
    z, psi = 1.0 - 2.0 * rng.random(n), 2.0 * np.pi * rng.random(n)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    wi = np.stack([r * np.cos(psi), r * np.sin(psi), z], axis=1).astype(np.float32)
    u = np.minimum(rng.random((n, 3)).astype(np.float32), np.nextafter(np.float32(1.0), np.float32(0.0)))
    if name.startswith("mix"):
        u[:, 0] *= np.float32(0.3 if name == "mix" else 0.6)
    bary = rng.random((n, 2))
    fold = bary.sum(axis=1) > 1.0
    bary[fold] = 1.0 - bary[fold]
    bary = (0.05 + 0.85 * bary).astype(np.float32)  # away from the edges: a traced ray finds the same triangle
    for a in (wo, wi, u, bary):
        a.setflags(write=False)
    prim = (np.arange(n) % 2).astype(np.uint32)
    prim.setflags(write=False)
    return {"wo": wo, "wi": wi, "u": u, "prim": prim, "bary": bary}


@functools.lru_cache(maxsize=None)
def sample_b_inputs(name: str) -> dict:
    """inputs(name) of a Mix material with other lobe numbers: u_lobe uniform in [ratio of the root, 1), the root's "sample b" branch (the
    inner nodes of the trees take either branch, as they do for inputs(name)); everything else, the records' points included, is shared"""
    inp = dict(inputs(name))
    rng = np.random.default_rng([SEED + 1, list(MATERIALS).index(name)])
    ratio = MIX_ROOT_RATIO[name]
    u = inp["u"].copy()
    u[:, 0] = np.clip((ratio + (1.0 - ratio) * rng.random(COUNT)).astype(np.float32), np.float32(ratio), np.nextafter(np.float32(1.0), np.float32(0.0)))
    u.setflags(write=False)
    inp["u"] = u
    return inp


def points(name: str) -> np.ndarray:
    """float64 [N, 3]: the points of QUAD's quad the records of inputs(name) stand on (prim 0: vertices 0, 1, 2; prim 1: vertices 0, 2, 3)"""
    inp = inputs(name)
    v = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [1.0, 1.0, 0.0], [-1.0, 1.0, 0.0]])
    b = inp["bary"].astype(np.float64)
    second = inp["prim"] == 1
    v1, v2 = np.where(second[:, None], v[2], v[1]), np.where(second[:, None], v[3], v[2])
    return (1.0 - b[:, 0:1] - b[:, 1:2]) * v[0] + b[:, 0:1] * v1 + b[:, 1:2] * v2


def hit_records(name: str) -> np.ndarray:
    """[N, 8] float32 lrhip_ray_hit records for inputs(name), made by hand: inst 0, tri = LR_INVALID_ID (the instance path)"""
    inp = inputs(name)
    rec = np.zeros((COUNT, 8), np.float32)
    ids = rec.view(np.uint32)
    rec[:, 0] = 1.0
    rec[:, 1:3] = inp["bary"]
    ids[:, 3], ids[:, 4], ids[:, 5] = 0, inp["prim"], INVALID
    return rec


def rays(name: str) -> np.ndarray:
    """[N, 8] float32 rays that see the records' points from wo: o = p + wo, d = -wo (unit to rounding: taken bit for bit), [0, inf)"""
    inp = inputs(name)
    r = np.zeros((COUNT, 8), np.float32)
    r[:, 0:3] = (points(name) + inp["wo"].astype(np.float64)).astype(np.float32)
    r[:, 4:7] = -inp["wo"]
    r[:, 7] = np.inf
    return r


@functools.lru_cache(maxsize=None)
def oracle_answers(name: str) -> dict:
    """the oracle's answers for inputs(name): evaluate [N, 4] float32 (f, pdf) and sample [N, 8] (f, pdf, wi, event as a number)"""
    probe = SurfaceProbe(material_scene(name))
    inp = inputs(name)
    evaluate, sample = np.zeros((COUNT, 4), np.float32), np.zeros((COUNT, 8), np.float32)
    for k in range(COUNT):
        f, pdf = probe.evaluate(inp["wo"][k], inp["wi"][k])
        evaluate[k, 0:3], evaluate[k, 3] = f, pdf
        f, pdf, wi, event = probe.sample(inp["wo"][k], *(float(x) for x in inp["u"][k]))
        sample[k, 0:3], sample[k, 3], sample[k, 4:7], sample[k, 7] = f, pdf, wi, event
    evaluate.setflags(write=False)
    sample.setflags(write=False)
    return {"evaluate": evaluate, "sample": sample}


@functools.lru_cache(maxsize=None)
def oracle_sample_b(name: str) -> np.ndarray:
    """the oracle's sample [N, 8] (f, pdf, wi, event as a number) for sample_b_inputs(name)"""
    probe = SurfaceProbe(material_scene(name))
    inp = sample_b_inputs(name)
    sample = np.zeros((COUNT, 8), np.float32)
    for k in range(COUNT):
        f, pdf, wi, event = probe.sample(inp["wo"][k], *(float(x) for x in inp["u"][k]))
        sample[k, 0:3], sample[k, 3], sample[k, 4:7], sample[k, 7] = f, pdf, wi, event
    sample.setflags(write=False)
    return sample


def excluded(name: str, mode: str) -> np.ndarray:
    """bool [N]: the records left out of the value comparison -- a function of the inputs and the oracle's answer only.  At grazing incidence
    the closures' side tests (same hemisphere, validate_surface_sides, reflect or refract) flip on the last bit of a cosine, so a record is
    left out where |wo.z|, the given |wi.z| (evaluate) or the direction the ORACLE sampled (sample, where it sampled one: pdf > 0) has
    |z| < GRAZING.  mode: "evaluate", "sample", or "sample_b" for sample_b_inputs(name)"""
    inp = inputs(name)
    out = np.abs(inp["wo"][:, 2]) < GRAZING
    if mode == "evaluate":
        return out | (np.abs(inp["wi"][:, 2]) < GRAZING)
    sample = oracle_sample_b(name) if mode == "sample_b" else oracle_answers(name)["sample"]
    return out | ((sample[:, 3] > 0.0) & (np.abs(sample[:, 6]) < GRAZING))


def relative_error(dev, ref) -> np.ndarray:
    """componentwise |dev - ref| / max(|ref|, 1e-2), in float64"""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    return np.abs(dev - ref) / np.maximum(np.abs(ref), 1e-2)


def invalid_record() -> np.ndarray:
    """the invalid record as 8 words: zeros, except event = LR_INVALID_ID"""
    r = np.zeros(8, np.uint32)
    r[7] = INVALID
    return r
