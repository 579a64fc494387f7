"""CPU test: tools/host_ownership_check.cpp, a program of its own over the C ABI's scene and context ownership, built with the host
sanitizers (make host_ownership_check) and run as a child process with leak detection on.  Nothing of it is loaded into this
process and nothing is preloaded: the program is instrumented itself."""
import os
import subprocess

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "minipath_amd", "csrc")


def test_scene_and_context_ownership_under_the_host_sanitizers():
    """Host-only scenes, a group and an instance set of them, materials on a member and on the group, members destroyed before
    the groups, then mp_ctx_create where no device is visible: exit status 0, "ok", and no sanitizer or leak report."""
    subprocess.run(["make", "-C", CSRC, "-j", "8", "host_ownership_check"], check=True, capture_output=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    env["HIP_VISIBLE_DEVICES"] = env["ROCR_VISIBLE_DEVICES"] = ""  # mp_ctx_create must fail cleanly: the program opens no device
    r = subprocess.run([os.path.join(CSRC, "host_ownership_check")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "host_ownership_check: ok", r.stdout
    assert lines[-2].startswith("host_ownership_check: mp_ctx_create returned ") and int(lines[-2].split()[-1]) != 0, r.stdout
    for word in ("Sanitizer", "runtime error", "ERROR:", "leak"):
        assert word not in r.stderr, r.stderr
