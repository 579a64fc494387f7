"""The dispatch census (no GPU): the kernel table (minipath_amd/csrc/kernel_table.h, read from the built probe libmp_plan_probe.so) is
exactly the set of rows of tests/dispatch_cases.py, which tests/test_gpu_dispatch_matrix.py runs one by one; the library launches
in one place only, the switch the table generates (family_launch.h), which records the row's name and which every translation unit
expands over the sub-tables of its own kernels; and no instantiation of a kernel template is named outside the table.  A new instantiation without a parity case, or a case whose instantiation is gone, fails here, on every machine."""
import ctypes as C
import os
import re
import shutil
import subprocess

from tests import dispatch_cases as dc
from tests import plan_probe as pp
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "minipath_amd", "csrc")
RAW_LAUNCH = r"\bhipLaunchKernelGGL\b|<<<|\bhipLaunchKernel\b|\bhipModuleLaunchKernel\b|\bhipExtLaunchKernelGGL\b"


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _library_sources():
    return {f: _strip_comments(open(os.path.join(CSRC, f)).read()) for f in sorted(os.listdir(CSRC))
            if f.endswith((".cpp", ".h", ".hip")) and f not in dc.PROBE_FILES}


def census(names):
    """what separates a kernel table from the case table: (instantiations without a case, cases without an instantiation)"""
    assert len(names) == len(set(names)), "no instantiation has two rows"
    for name, why in dc.EXCLUDED.items():
        assert name in names and why, f"{name} is excluded but no longer in the table"
    table, cases = set(names) - set(dc.EXCLUDED), set(dc.CASES)
    return sorted(table - cases), sorted(cases - table)


def test_the_case_table_is_the_census():
    assert census(pp.table()) == ([], [])
    # the names are the rows as written, the MP_MCACHE_WPE position at its default
    for n in ("render_tiles_packet_kernel<16, true, 7>", "render_tiles_packet_kernel<32, false, 8, false, true>", "render_paths_kernel<2, true, false>",
              "render_aov_packet_kernel<16, false, 8, false, true>", "query_rays_kernel<true, kAnyHit>", "wf_scan_kernel"):
        assert n in pp.table(), n
    assert not [n for n in pp.table() if "MP_" in n or "  " in n]


def _device_sources():
    """the sources with device code: the translation units and the headers they share"""
    src = _library_sources()
    return {f: t for f, t in src.items() if f.endswith(".hip") or "__device__" in t or "__global__" in t}


def _subtables():
    """{sub-table macro: [row ids]} and the order MP_KERNEL_TABLE concatenates them in, from kernel_table.h"""
    text = _library_sources()["kernel_table.h"]
    subs = {m.group(1): re.findall(r"\bX\((K_\w+),\s*(.*?)\)\s", m.group(2))
            for m in re.finditer(r"#define (MP_KERNELS_\w+)\(X\)((?:[^\n]*\\\n)*[^\n]*\n)", text)}
    whole = re.search(r"#define MP_KERNEL_TABLE\(X\)((?:[^\n]*\\\n)*[^\n]*\n)", text).group(1)
    return subs, re.findall(r"(MP_KERNELS_\w+)\(X\)", whole)


def test_no_launch_bypasses_the_record():
    src = _library_sources()
    raw = [(f, m.start()) for f, t in src.items() for m in re.finditer(RAW_LAUNCH, t)]
    assert len(raw) == 1 and raw[0][0] == "family_launch.h", "the library launches only inside the MP_LAUNCH macro"
    text = src["family_launch.h"]
    line = text[: raw[0][1]].count("\n")
    window = "\n".join(text.split("\n")[line - 3: line + 1])
    assert "#define MP_LAUNCH(" in window and "note_launch(id)" in window, "the one raw launch is MP_LAUNCH's own, next to its record"
    uses = [(f, m.start()) for f, t in src.items() for m in re.finditer(r"\bMP_LAUNCH\(", t)
            if "#define" not in t[t.rfind("\n", 0, m.start()):m.start()]]
    assert len(uses) == 1 and uses[0][0] == "family_launch.h", "MP_LAUNCH is used once: by the switch over a sub-table"
    at = text[: uses[0][1]].count("\n")
    around = "\n".join(text.split("\n")[at - 3: at + 14])
    assert "#define MP_LAUNCH_ROW(row, ...)" in around and "case row:" in around and "SUBTABLE(MP_LAUNCH_ROW)" in around, "... generated from the table, row by row"
    assert len(re.findall(r"\bMP_LAUNCH_ROW\b", "".join(src.values()))) == 2, "the row's case is written once and expanded by MP_FAMILY_LAUNCHER alone"
    for f in dc.PROBE_FILES:
        assert os.path.exists(os.path.join(CSRC, f)), f"{f} is excluded but gone"


def test_the_subtables_are_the_table_and_every_unit_launches_its_own():
    subs, order = _subtables()
    assert sorted(order) == sorted(subs) and len(order) == len(set(order)), "MP_KERNEL_TABLE is every sub-table once"
    rows = [r for name in order for r in subs[name]]
    ids = [i for i, _ in rows]
    assert len(ids) == len(set(ids)), "... with each row once"
    assert [k.replace("MP_MCACHE_WPE", "8") for _, k in rows] == pp.table(), "... and it is the table the library was built from, in its order"
    # every translation unit expands the switch once, over the sub-table of its own family
    src = _library_sources()
    units = {}
    for f, t in src.items():
        for name in re.findall(r"^MP_FAMILY_LAUNCHER\((\w+)\)", t, flags=re.M):
            assert f.endswith(".hip") and f not in units and name in subs, (f, name)
            units[f] = [name]
    assert units == {"kernels.hip": ["MP_KERNELS_UTILITIES"], "kernels_tiles.hip": ["MP_KERNELS_TILES"], "kernels_aov.hip": ["MP_KERNELS_AOV"],
                     "kernels_paths.hip": ["MP_KERNELS_PATHS"], "kernels_staged.hip": ["MP_KERNELS_STAGED"],
                     "kernels_queries.hip": ["MP_KERNELS_QUERIES"]}
    assert not [f for f, t in src.items() if "MP_KERNELS_HERE" in t], "no unit concatenates sub-tables of its own any more"
    # ... every sub-table is expanded exactly once in the library
    assert sorted(n for names in units.values() for n in names) == sorted(subs), units
    # ... by the unit that defines the sub-table's kernels, which defines no others
    for f, names in units.items():
        kernels = set(re.findall(r"__global__ [^\n]*\bvoid (\w+)\(", src[f]))
        assert {k.split("<")[0] for n in names for _, k in subs[n]} == kernels, (f, names)


def test_kernel_templates_are_instantiated_by_the_table_alone():
    src = _library_sources()
    device = "\n".join(_device_sources().values())
    templates = set(re.findall(r"^template <[^\n]*>\n__global__ [^\n]*\bvoid (\w+)\(", device, flags=re.M))
    assert {"render_tiles_packet_kernel", "render_paths_kernel", "render_aov_packet_kernel", "wf_camera_kernel", "query_rays_kernel"} <= templates
    assert {n.split("<")[0] for n in pp.table() if "<" in n} == templates, "every kernel template has rows, and only kernel templates have arguments"
    for f, t in src.items():
        if f != "kernel_table.h":
            named = [k for k in templates if re.search(r"\b%s\s*<" % k, t)]
            assert not named, (f, named)


def test_rows_are_well_formed():
    rows = list(dc.CASES.items()) + [(k, r) for k, r in dc.GATES.values()] + [(None, r) for r, _ in dc.RAGGED.values()]
    for name, row in rows:
        assert set(row["opts"]) <= set(dc.DEFAULTS), name
        assert row["api"] in ("render", "paths", "wf", "aov", "trace", "bounded", "occluded", "rays", "untile", "async")
        assert row["scene"].partition("+")[0] in dc.FACTS, name
        for other in row["also"]:
            assert other in dc.CASES, (name, other)
    for expected, _ in dc.GATES.values():
        assert expected in dc.CASES and "false, true>" not in expected, expected  # an uncached name
    for row, passes in dc.RAGGED.values():
        assert sum(n for n, _ in passes) == row["spp"] and len({k for _, k in passes}) >= 4
        assert all(k in dc.CASES for _, k in passes)


def _table_of(tmp_path, tag, edit):
    """the names of a probe built from a copy of the sources whose kernel_table.h went through edit()"""
    inc, work = tmp_path / tag / "include", tmp_path / tag / "pkg" / "csrc"  # mp_internal.h includes ../../include/minipath_hip.h
    inc.mkdir(parents=True)
    work.mkdir(parents=True)
    shutil.copy(os.path.join(ROOT, "include", "minipath_hip.h"), inc)
    for f in ("launch_plan.cpp", "launch_plan.h", "plan_probe.cpp", "mp_internal.h", "kernel_table.h"):
        shutil.copy(os.path.join(CSRC, f), work)
    table = work / "kernel_table.h"
    before = table.read_text()
    after = edit(before)
    assert after != before
    table.write_text(after)
    cxx = os.environ.get("HOSTCXX") or next(c for c in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("c++")) if c and os.path.exists(c))
    so = str(work / "probe.so")
    subprocess.run([cxx, "-O0", "-std=c++17", "-fPIC", "-shared", "-o", so, "plan_probe.cpp", "launch_plan.cpp"], cwd=work, check=True)
    L = C.CDLL(so)
    L.mp_plan_kernel_name.restype = C.c_char_p
    return [L.mp_plan_kernel_name(i).decode() for i in range(L.mp_plan_kernel_count())]


def test_a_changed_launcher_is_noticed(tmp_path):
    """the census on probes built from edited copies of the list: a row added, a row taken out"""
    at = "    X(K_PACKET_1,              render_tiles_packet_kernel<1, false, 7>)                             \\\n"
    added = _table_of(tmp_path, "added", lambda s: s.replace(at, at + "    X(K_PACKET_128, render_tiles_packet_kernel<128, false, 7>) \\\n"))
    assert census(added) == (["render_tiles_packet_kernel<128, false, 7>"], [])
    row = "    X(K_QUANTISE,              quantise_kernel)\n"
    gone = _table_of(tmp_path, "gone", lambda s: s.replace("untile_kernel)                                                       \\\n" + row,
                                                           "untile_kernel)\n"))
    assert census(gone) == ([], ["quantise_kernel"])
