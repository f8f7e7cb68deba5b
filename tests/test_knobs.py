"""The environment knobs the native code reads are exactly the ones README's knob table documents, and none of the
retired experiment build switches is left in the kernels."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = r"(?:ZIP_HIP|ZINC_HOST)_[A-Z0-9_]+"


def _sources(*patterns):
    return [p for pat in patterns for p in sorted(glob.glob(os.path.join(ROOT, pat)))]


def _read(path):
    with open(path) as fh:
        return fh.read()


def test_knobs_read_match_the_readme_table():
    # every knob is read by name: getenv("...") or env_long("...", ...) in the library, os.environ.get("...") in Python
    read = set()
    for path in _sources("zinc_amd/csrc/*.hip", "zinc_amd/host/*.cpp", "zinc_amd/*.py"):
        read |= set(re.findall(r'(?:getenv|env_long|environ\.get)\(\s*"(' + KNOB + r')"', _read(path)))
    readme = _read(os.path.join(ROOT, "README.md"))
    table = readme.split("## Environment knobs", 1)[1].split("\n## ", 1)[0]
    documented = set()
    for line in table.splitlines():
        if line.startswith("| `"):
            documented |= set(re.findall(r"`(" + KNOB + r")", line.split(" | ", 1)[0]))
    assert read, "no knob found in the sources: the pattern no longer matches how they are read"
    assert read - documented == set(), "read by the code but missing from README's knob table"
    assert documented - read == set(), "in README's knob table but read by nothing"


def test_no_experiment_switches_in_the_kernels():
    prefix = "ZIPK_" + "EXP_"  # (split: a grep for the prefix over the tree stays empty)
    hits = [os.path.relpath(p, ROOT) for p in _sources("zinc_amd/csrc/*") if prefix in _read(p)]
    assert hits == []


def test_schedule_and_gather_knobs_are_read_by_zip_ctx_create_only():
    """tests/test_gpu_gather_variants.py sets these per test, in process, before it makes its context: each is read in
    exactly one place, inside zip_ctx_create -- a `static const` read anywhere else would pin the first test's value."""
    src = _read(os.path.join(ROOT, "zinc_amd", "csrc", "zip_hip.hip"))
    start = src.index("int32_t zip_ctx_create(")
    body = src[start:src.index("\nvoid zip_ctx_destroy(", start)]
    for knob in ("ZIP_HIP_CHUNKS", "ZIP_HIP_CHUNK_ROUNDS", "ZIP_HIP_GATHER_RPB", "ZIP_HIP_GATHER_STREAM", "ZIP_HIP_NO_COMPACT_ROWS"):
        reads = re.findall(r'(?:getenv|env_long)\(\s*"' + knob + '"', src)
        assert len(reads) == 1, (knob, len(reads))
        assert len(re.findall(r'(?:getenv|env_long)\(\s*"' + knob + '"', body)) == 1, knob
