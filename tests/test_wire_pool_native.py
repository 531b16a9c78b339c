"""`native/wire_pool.hpp` and `wire::ResponseReader` as a stand-alone
program under ASan + UBSan, against a loopback listener of its own."""

import os
import subprocess

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NATIVE_DIR = os.path.join(REPO, "k8s_operator_libs_amd", "native")


def test_wire_pool_selftest_under_sanitizers(tmp_path):
    exe = tmp_path / "wire_pool_selftest"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-pthread", f"-I{NATIVE_DIR}",
         os.path.join(REPO, "tests", "native", "wire_pool_selftest.cpp"),
         "-o", str(exe)],
        capture_output=True, text=True, timeout=300,
    )
    assert build.returncode == 0, build.stderr
    # the instrumented code is the program itself; ASan only has to accept
    # whatever library order the inherited environment gives it
    env = dict(os.environ)
    for name, extra in (
            ("ASAN_OPTIONS", "verify_asan_link_order=0"),
            ("UBSAN_OPTIONS", "halt_on_error=1:print_stacktrace=1")):
        env[name] = ":".join(v for v in (env.get(name), extra) if v)
    run = subprocess.run([str(exe)], capture_output=True, text=True,
                         timeout=120, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "checks passed" in run.stdout
