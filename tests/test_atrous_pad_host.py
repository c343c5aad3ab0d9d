"""csrc/pass_core.h atrous_resident_pad (the residency cap of kf_shadows_atrous01) without a GPU: a stand-alone program with its own main
(tests/atrous_pad_check.cpp), built with the address and undefined-behaviour sanitizers; nothing is loaded into Python.  For LDS sizes of
64-160 KiB per CU, static sizes of 0-40 000 B and R = 3-8: floor(LDS / (static + pad)) == R wherever R workgroups of the kernel's own LDS fit
at all, static + pad within the 64 KiB a workgroup may ask for, and no pad where the kernel alone already allows R or fewer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybrid_rendering_amd", "csrc")


def test_pad_gives_exactly_r_workgroups_per_cu(tmp_path):
    exe = str(tmp_path / "atrous_pad_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "atrous_pad_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1 and lines[0].startswith("pad: ") and lines[0].endswith(" 0 failed"), r.stdout
    assert int(lines[0].split()[1]) > 10000, "the sweep must have run"
