"""The host-side core the three denoised passes share (csrc/pass_core.h), without a GPU: its plain part — pass rows under the two band rules, the
geometry-record state machine — in a stand-alone program under the address and undefined-behaviour sanitizers (tests/pass_core_check.cpp: a
binary of its own, nothing is loaded into Python).  The expected values there are literals derived by hand from the three passes' own copies of
this logic, as they were before they shared it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid_rendering_amd", "csrc")


def test_rows_and_records_under_sanitizers(tmp_path):
    exe = str(tmp_path / "pass_core_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "pass_core_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0] == "rows: 23 checks" and lines[1] == "records: 41 checks", r.stdout


def test_the_plain_part_needs_no_hip_header():
    """what the stand-alone program compiles must stay free of the HIP runtime: PassCore and its helpers sit behind __HIPCC__"""
    text = open(os.path.join(CSRC, "pass_core.h")).read()
    plain, _, hip = text.partition("#ifdef __HIPCC__")
    assert hip and "#include <hip" not in plain and "hr_internal.h" not in plain and "struct PassRows" in plain and "struct GeoRecords" in plain
    assert "struct PassCore" in hip
