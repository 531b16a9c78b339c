"""The generator and host reference of the vector-ALU check
(`native/valu_problems.hpp`) as a stand-alone program under ASan + UBSan: no
GPU, no Python extension, nothing preloaded."""

import os
import subprocess

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NATIVE_DIR = os.path.join(REPO, "k8s_operator_libs_amd", "native")


def test_valu_problems_selftest_under_sanitizers(tmp_path):
    exe = tmp_path / "valu_problems_selftest"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=all", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "valu_problems_selftest.cpp"),
         "-o", str(exe)],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr
    # the inherited environment stays as it is; the instrumented code is the
    # program itself, so ASan only needs to accept whatever library order
    # that environment gives it
    env = dict(os.environ)
    for name, extra in (
            ("ASAN_OPTIONS", "verify_asan_link_order=0"),
            ("UBSAN_OPTIONS", "halt_on_error=1:print_stacktrace=1")):
        env[name] = ":".join(v for v in (env.get(name), extra) if v)
    run = subprocess.run([str(exe)], capture_output=True, text=True,
                         timeout=120, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "checks passed" in run.stdout
