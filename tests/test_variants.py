"""The A/B variant table (ramcloud_amd/variants.py) and the RAMCRC_LIB guard:
every variant moves a knob that the sources define and use away from its
default, and no variant -- nor any library loaded through RAMCRC_LIB -- names a knob
that gave wrong results (build.UNSAFE_DEFINES).  CPU only."""
import glob
import os
import re

import pytest

from ramcloud_amd import build, ramcrc
from ramcloud_amd.variants import VARIANTS

CSRC = os.path.join(os.path.dirname(build.__file__), "csrc")


def _sources():
    return "".join(open(f).read() for f in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(f))


KNOB_DEF = r"#ifndef (RAMCRC_\w+)\n(?://[^\n]*\n)*#define \1 (\S+)"


def _knob_uses(src, knob):
    """Occurrences of `knob` in code: outside its own #ifndef/#define pair and
    outside comments (a knob that only its definition or prose names moves
    nothing)."""
    code = re.sub(KNOB_DEF.replace(r"(RAMCRC_\w+)", "(%s)" % knob) + r"[^\n]*", "", src)
    code = re.sub(r"//[^\n]*|/\*.*?\*/", "", code, flags=re.S)
    return re.findall(r"\b%s\b" % knob, code)


def test_knob_use_detection():
    src = "#ifndef RAMCRC_A\n// why\n#define RAMCRC_A 1   // RAMCRC_A\n#endif\n// RAMCRC_A in prose\n"
    assert dict(re.findall(KNOB_DEF, src)) == {"RAMCRC_A": "1"}
    assert not _knob_uses(src, "RAMCRC_A")
    assert not _knob_uses(src + "int x = RAMCRC_AB;\n", "RAMCRC_A")
    assert _knob_uses(src + "#if RAMCRC_A\n#endif\n", "RAMCRC_A")
    assert _knob_uses(src + "constexpr int kA = RAMCRC_A;\n", "RAMCRC_A")


def test_variant_knobs_exist_and_move():
    src = _sources()
    defaults = dict(re.findall(KNOB_DEF, src))
    for name, defs in VARIANTS.items():
        assert defs, name
        for d in defs:
            k, v = d.split("=")
            assert k in defaults, f"{name}: {k} is not a knob of the sources"
            assert defaults[k] != v, f"{name}: {d} is the default"
            assert _knob_uses(src, k), f"{name}: {k} is defined but nothing uses it"


def test_no_unsafe_variant_and_build_refuses(tmp_path):
    for name, defs in VARIANTS.items():
        assert not build.unsafe_defines(defs), name
    out = tmp_path / "variants" / "lib.so"
    with pytest.raises(ValueError):
        build._compile(str(out), ("RAMCRC_PROBE_FOLD=1",))
    assert not out.parent.exists()   # refused before anything was created


def test_build_info_defines_parsed():
    assert ramcrc.build_defines("ramcrc gfx950 src_sha=0123 part_shift=16 defines=none") == []
    info = "ramcrc gfx950 src_sha=0123 defines=RAMCRC_PU=3,RAMCRC_WALK_DEBUG=1"
    assert ramcrc.build_defines(info) == ["RAMCRC_PU=3", "RAMCRC_WALK_DEBUG=1"]
    assert build.unsafe_defines(ramcrc.build_defines(info)) == ["RAMCRC_WALK_DEBUG=1"]


def test_product_library_reports_no_defines():
    if not os.path.exists(build.LIB):
        pytest.skip("library not built")
    blob = open(build.LIB, "rb").read()
    assert b" defines=none" in blob
