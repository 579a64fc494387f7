"""The dispatch census (no GPU): every kernel launch of minipath_amd/csrc/kernels.hip goes through the recording macro MP_LAUNCH, and
the set of instantiation names those sites can launch -- read from the source, the small launch macros expanded -- is exactly the
set of rows of tests/dispatch_cases.py, which tests/test_gpu_dispatch_matrix.py runs one by one.  A new instantiation without a
parity case, or a case whose instantiation is gone, fails here, on every machine."""
import os
import re


from tests import dispatch_cases as dc
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "minipath_amd", "csrc")


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _call_args(text, pos):
    """the top-level, comma-separated arguments of the call whose '(' is at pos, and the index after its ')'"""
    assert text[pos] == "("
    depth, args, cur, i = 0, [], "", pos
    while True:
        ch = text[i]
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                args.append(cur.strip())
                return args, i + 1
        if ch == "," and depth == 1:
            args.append(cur.strip())
            cur = ""
        elif not (depth == 1 and ch == "(" and i == pos):
            cur += ch
        i += 1


def _defines(text):
    """{name: (params or None, body)} of the #define lines, continuation lines joined"""
    out = {}
    joined = re.sub(r"\\\n", " ", text)
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(\(([^)]*)\))?[ \t]*(.*)$", joined, flags=re.M):
        params = [p.strip() for p in m.group(3).split(",")] if m.group(2) else None
        out.setdefault(m.group(1), (params, m.group(4).strip()))
    return out


def _normal(name):
    """the preprocessor's stringification of the kernel argument, as launch_log_text() reports it"""
    name = re.sub(r"\s+", " ", name.strip())
    if name.startswith("(") and name.endswith(")"):
        name = name[1:-1].strip()
    return re.sub(r"\s*,\s*", ", ", name)


def launch_sites(path):
    return launch_sites_of(open(path).read())


def launch_sites_of(source):
    """Names of every kernel the source launches through MP_LAUNCH, its launch macros (macros whose body launches) expanded at their
    uses and object-like macros inside the template arguments (MP_MCACHE_WPE) replaced by their default."""
    text = _strip_comments(source)
    defs = _defines(text)
    launchers = {n: d for n, d in defs.items() if n != "MP_LAUNCH" and d[0] is not None and "MP_LAUNCH(" in d[1]}
    consts = {n: d[1] for n, d in defs.items() if d[0] is None and re.fullmatch(r"\d+", d[1] or "")}
    body = re.sub(r"\\\n", " ", text)
    body = re.sub(r"^[ \t]*#[ \t]*define[^\n]*$", "", body, flags=re.M)  # uses only: the definitions were read above
    for _ in range(4):  # launch macros do not nest deeper
        for name, (params, mbody) in launchers.items():
            while True:
                m = re.search(r"\b%s\(" % name, body)
                if not m:
                    break
                args, end = _call_args(body, m.end() - 1)
                if params and params[-1] == "...":
                    fixed = params[:-1]
                    args = args[:len(fixed)] + [", ".join(args[len(fixed):])]
                    names = fixed + ["__VA_ARGS__"]
                else:
                    names = params
                assert len(args) == len(names), (name, args)
                exp = mbody
                for p, a in zip(names, args):
                    exp = re.sub(r"\b%s\b" % p, a, exp)
                body = body[:m.start()] + exp + body[end:]
    names = []
    for m in re.finditer(r"\bMP_LAUNCH\(", body):
        args, _ = _call_args(body, m.end() - 1)
        k = args[0]
        for c, v in consts.items():
            k = re.sub(r"\b%s\b" % c, v, k)
        names.append(_normal(k))
    return names


def test_no_launch_bypasses_the_record():
    text = _strip_comments(open(os.path.join(CSRC, "kernels.hip")).read())
    raw = [m.start() for m in re.finditer(r"\bhipLaunchKernelGGL\b|<<<|\bhipLaunchKernel\b|\bhipModuleLaunchKernel\b|\bhipExtLaunchKernelGGL\b", text)]
    assert len(raw) == 1, "kernels.hip launches only inside the MP_LAUNCH macro"
    line = text[: raw[0]].count("\n")
    window = "\n".join(text.split("\n")[line - 4: line + 1])
    assert "#define MP_LAUNCH(" in window and "note_launch(MP_STR(kernel))" in window, "the one raw launch is MP_LAUNCH's own, next to its record"
    # the other sources of the library launch nothing
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".cpp", ".h", ".hip")) and f != "kernels.hip" and f not in dc.PROBE_FILES:
            t = _strip_comments(open(os.path.join(CSRC, f)).read())
            assert not re.search(r"\bhipLaunchKernelGGL\b|<<<|\bMP_LAUNCH\(", t), f
    for f in dc.PROBE_FILES:
        assert os.path.exists(os.path.join(CSRC, f)), f"{f} is excluded but gone"


def test_the_case_table_is_the_census():
    sites = launch_sites(os.path.join(CSRC, "kernels.hip"))
    assert len(sites) == len(set(sites)), "no instantiation is launched from two sites"
    parsed = set(sites)
    for name, why in dc.EXCLUDED.items():
        assert name in parsed and why, f"{name} is excluded but no longer launched"
    census = parsed - set(dc.EXCLUDED)
    table = set(dc.CASES)
    assert table == census, {"instantiations without a case": sorted(census - table), "cases without an instantiation": sorted(table - census)}


def test_the_parser_sees_what_the_preprocessor_sees():
    """spot checks of the expansion: nested launch macros, variadic template arguments, an object-like macro in the arguments"""
    sites = set(launch_sites(os.path.join(CSRC, "kernels.hip")))
    for n in ("render_tiles_packet_kernel<16, true, 7>", "render_tiles_packet_kernel<32, false, 8, false, true>", "render_paths_kernel<2, true, false>",
              "render_aov_packet_kernel<16, false, 8, false, true>", "query_rays_kernel<true, kAnyHit>", "wf_scan_kernel"):
        assert n in sites, n
    assert not [n for n in sites if "SV" in n or "__VA_ARGS__" in n or "MP_" in n]


def test_rows_are_well_formed():
    rows = list(dc.CASES.items()) + [(k, r) for k, r in dc.GATES.values()] + [(None, r) for r, _ in dc.RAGGED.values()]
    for name, row in rows:
        assert set(row["opts"]) <= set(dc.DEFAULTS), name
        assert row["api"] in ("render", "paths", "wf", "aov", "trace", "bounded", "occluded", "rays", "untile", "async")
        for other in row["also"]:
            assert other in dc.CASES, (name, other)
    for expected, _ in dc.GATES.values():
        assert expected in dc.CASES and "false, true>" not in expected, expected  # an uncached name
    for row, passes in dc.RAGGED.values():
        assert sum(n for n, _ in passes) == row["spp"] and len({k for _, k in passes}) >= 4
        assert all(k in dc.CASES for _, k in passes)


def test_a_changed_launcher_is_noticed():
    """the parser on edited copies of the source: a new site written plainly, a new use of a launch macro, a site taken out"""
    src = open(os.path.join(CSRC, "kernels.hip")).read()
    census = set(launch_sites_of(src))
    at = "    else MP_LAUNCH_PACKET(1, 7);\n"
    assert src.count(at) == 1
    plain = src.replace(at, at + "    MP_LAUNCH((render_tiles_packet_kernel<128, false, 7>), dim3(grid), dim3(256), 0, st, P);\n")
    assert set(launch_sites_of(plain)) - census == {"render_tiles_packet_kernel<128, false, 7>"}
    macro = src.replace(at, at + "    MP_LAUNCH_PACKET(128, 5);\n")
    assert set(launch_sites_of(macro)) - census == {"render_tiles_packet_kernel<128, true, 5>", "render_tiles_packet_kernel<128, false, 5>"}
    gone = src.replace("MP_LAUNCH(wf_scan_kernel,", "launch_elsewhere(wf_scan_kernel,")
    assert census - set(launch_sites_of(gone)) == {"wf_scan_kernel"}
