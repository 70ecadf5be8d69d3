"""The library's translation units (the Makefile's UNITS): every entry point of rt3.h is defined in exactly one of them, the render unit and the scene
unit include none of each other's kernel headers, and csrc/rt3_scene.hpp — what rt3_device.hip calls in rt3_scene.hip — stands alone.  No GPU."""
import os
import re
import subprocess

from test_abi import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "raytracer-3_amd")
CSRC = os.path.join(PKG, "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def units():
    """The Makefile's UNITS, as paths."""
    text = open(os.path.join(PKG, "Makefile")).read()
    line = re.search(r"^UNITS\s*:=\s*(.+)$", text, re.M).group(1)
    return [os.path.join(PKG, u) for u in line.split()]


def includes(name):
    return re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', open(os.path.join(CSRC, name)).read(), re.M)


def defined_in(text, name):
    """Definitions of the function `name` in a source text: at the start of a line a return type, the name, a balanced parameter list and a `{`."""
    count = 0
    for m in re.finditer(r'^(?:extern "C" )?[A-Za-z_][\w \*]*?\b%s\s*\(' % re.escape(name), text, re.M):
        depth, i = 1, m.end()
        while depth and i < len(text):
            depth += (text[i] == "(") - (text[i] == ")")
            i += 1
        count += text[i:].lstrip().startswith("{")
    return count


def test_every_entry_point_is_defined_in_exactly_one_unit():
    paths = units()
    assert os.path.join(PKG, "csrc", "rt3_device.hip") in paths and os.path.join(PKG, "csrc", "rt3_scene.hip") in paths
    text = {p: re.sub(r"//[^\n]*", "", open(p).read()) for p in paths}
    declared = header_symbols()
    assert len(declared) >= 130
    for name in declared:
        where = {os.path.basename(p): defined_in(t, name) for p, t in text.items() if defined_in(t, name)}
        assert sum(where.values()) == 1, (name, where)


def test_render_unit_includes_no_scene_header():
    got = includes("rt3_device.hip")
    for header in ("hipcub/hipcub.hpp", "rt3_scene_kernels.hpp", "rt3_regroup.hpp", "rt3_scene_build.hpp", "rt3_env_table.hpp", "rt3_light_table.hpp",
                   "rt3_sphere_plan.hpp"):
        assert header not in got, header
    assert not [h for h in got if "hipcub" in h]


def test_scene_unit_includes_no_trace_kernel_header():
    got = includes("rt3_scene.hip")
    for header in ("rt3_matrix_filter.hpp", "rt3_path.hpp", "rt3_valu_scan.hpp", "rt3_level_filter.hpp", "rt3_reduce.hpp", "rt3_adaptive.hpp", "rt3_aov.hpp",
                   "rt3_lens.hpp", "rt3_primary_lists.hpp"):
        assert header not in got, header


def test_kernel_headers_belong_to_one_unit():
    """A header that defines a kernel is included by one unit; rt3_shared_kernels.hpp is the exception DESIGN.md names."""
    by_header = {}
    for unit in units():
        for h in includes(os.path.basename(unit)):
            if os.path.exists(os.path.join(CSRC, h)) and "__global__" in open(os.path.join(CSRC, h)).read():
                by_header.setdefault(h, []).append(os.path.basename(unit))
    shared = sorted(h for h, u in by_header.items() if len(u) > 1)
    assert shared == ["rt3_shared_kernels.hpp"], by_header
    assert sorted(by_header["rt3_shared_kernels.hpp"]) == ["rt3_device.hip", "rt3_scene.hip"]
    assert "rt3_shared_kernels.hpp" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_scene_header_stands_alone(tmp_path):
    unit = tmp_path / "only_scene.hip"
    unit.write_text('#include "rt3_scene.hpp"\n'
                    "int probe(rt3_ctx* ctx, hipStream_t s) { int rc = check_scene(ctx); if (!rc) rc = ensure_env_table(ctx, s); return rc ? rc : ensure_light_table(ctx, s); }\n")
    # the Makefile's flags and include path, the host side only, no output (as test_ctx_header.py does for rt3_ctx.hpp)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-function",
                           "--cuda-host-only", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(unit)])
    text = open(os.path.join(CSRC, "rt3_scene.hpp")).read()
    assert re.findall(r'#include\s*[<"]([^>"]+)[>"]', text) == ["rt3_ctx.hpp"]
    code = re.sub(r"//[^\n]*", "", text)
    assert not re.search(r"\b(struct|class|union)\b", code)
    assert len(re.findall(r";", code)) <= 6                         # plain declarations, a handful: beyond that the cut is in the wrong place
