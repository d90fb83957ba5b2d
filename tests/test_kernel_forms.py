"""Source-text checks of how the kernels' code forms are selected (csrc/hip/kernel_forms.h) and of which compile-time switches exist.

No GPU and no build: the tests read the sources.  What they guard:
  (a) a kernel's feature mask becomes code forms in ONE header -- no other file under csrc/hip tests LR_VARIANT in a preprocessor condition
      (the two files that instantiate kernels from a mask, megapath_variant.hip and heavy_variant.hip, excepted);
  (b) the switches of settled experiments, retired with their alternatives, do not come back into the sources, the Makefile or the tools;
  (c) every macro that a build of the tree passes with -D is still read by the sources it is passed to.
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, "luisarender_amd", "csrc", "hip")
MASK_FILES = {"kernel_forms.h", "megapath_variant.hip", "heavy_variant.hip"}
RETIRED = [
    "LR_POOL_PARK_ON_STACK", "LR_POOL_FUSED_FETCH", "LR_POOL_FUSED_ALPHA", "LR_POOL_EARLY_TAIL_PRIO", "LR_POOL_STATE_LEAN", "LR_POOL_RAY_INIT",
    "LR_POOL_TURNOVER_MOVES", "LR_POOL_SINGLE", "LR_TRACE_PROBE", "LR_PADDED_DRAWS_OUT_OF_LINE", "LR_PROBE_NODE", "LR_PROBE_LEAF", "LR_PROBE_SHADE",
    "LR_SORT_COMPARATORS", "LR_WAVE_PRIORITIES", "LR_VOTE_BUILTIN", "LR_BAKED_SHADING", "LR_TEX_BY_VALUE", "LR_CALL_INLINE",
]
# the -D macros of the Makefile that go to the host compiler, and the sources that read them; every other one is a HIP build's
HOST_SIDE = {"LR_PLUGIN_IMPL": os.path.join("luisarender_amd", "csrc", "host"), "ORACLE_NUDGE_TRIG": "oracle"}


def files_under(*relative):
    for rel in relative:
        path = os.path.join(ROOT, rel)
        if os.path.isfile(path):
            yield path
            continue
        for base, dirs, names in os.walk(path):
            dirs[:] = [d for d in dirs if d != "__pycache__"]
            for name in sorted(names):
                if not name.endswith((".md", ".rst", ".txt", ".pyc", ".so", ".o")):
                    yield os.path.join(base, name)


def text_of(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def test_only_kernel_forms_turns_a_mask_into_code_forms():
    condition = re.compile(r"^\s*#\s*(if|elif)")
    offenders = []
    for path in files_under(os.path.join("luisarender_amd", "csrc", "hip")):
        if os.path.basename(path) in MASK_FILES:
            continue
        for number, line in enumerate(text_of(path).splitlines(), 1):
            if condition.match(line) and "LR_VARIANT" in line:
                offenders.append("%s:%d: %s" % (os.path.relpath(path, ROOT), number, line.strip()))
    assert not offenders, "preprocessor conditions on LR_VARIANT outside kernel_forms.h:\n" + "\n".join(offenders)
    assert os.path.isfile(os.path.join(HIP, "kernel_forms.h"))


def test_retired_switches_stay_retired():
    names = re.compile(r"\b(%s)\b" % "|".join(RETIRED))
    offenders = []
    for path in files_under(os.path.join("luisarender_amd", "csrc"), "include", "Makefile", "tools"):
        for number, line in enumerate(text_of(path).splitlines(), 1):
            found = names.search(line)
            if found:
                offenders.append("%s:%d: %s" % (os.path.relpath(path, ROOT), number, found.group(1)))
    assert not offenders, "retired compile-time switches named again:\n" + "\n".join(offenders)


def test_every_macro_a_build_defines_is_still_read():
    passed = set()
    for rel in ("Makefile", "__graft_entry__.py", os.path.join("tools", "stall_probe.py")):
        passed.update(re.findall(r"-D([A-Za-z_][A-Za-z0-9_]*)", text_of(os.path.join(ROOT, rel))))
    assert {"LR_VARIANT", "LR_HVARIANT", "LR_STALL_PROBE", "LR_POOL_EARLY_FETCH", "LR_STRAIGHT_TAIL", "LR_STACK_LDS", "LR_EXACT_LEAF"} <= passed, passed
    hip_text = "\n".join(text_of(p) for p in files_under(os.path.join("luisarender_amd", "csrc", "hip")))
    missing = []
    for name in sorted(passed):
        where = hip_text
        if name in HOST_SIDE and not re.search(r"\b%s\b" % name, hip_text):
            where = "\n".join(text_of(p) for p in files_under(HOST_SIDE[name]))
        if not re.search(r"\b%s\b" % name, where):
            missing.append(name)
    assert not missing, "passed with -D by a build, read by no source: %s" % ", ".join(missing)
