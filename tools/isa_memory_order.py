"""The order of a kernel's global reads (no GPU needed): every global_load, every s_waitcnt that waits on vmcnt, every s_barrier and every
loop (as the compiler marks its basic blocks) of the gfx950 assembly hipcc emits, in program order.
Dependent round trips show as load(s) -> wait -> load(s); a load inside `loop { ... }` is paid once per trip of that loop.
    python tools/isa_memory_order.py hybrid_rendering_amd/csrc/denoise_fast_shadows.hip 'kf_shadows_atrous01<16, true>'
HR_CFLAGS adds compiler flags, as in the build (e.g. HR_CFLAGS=-DFT_ATROUS01_TH=8 for another value of a knob)."""
import os, re, subprocess, sys, tempfile

src = sys.argv[1]
flt = sys.argv[2] if len(sys.argv) > 2 else ""
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hybrid_rendering_amd import build as hb

with tempfile.TemporaryDirectory() as td:
    flags = [f for f in hb.FLAGS if f not in ("-shared",)] + os.environ.get("HR_CFLAGS", "").split()
    out = os.path.join(td, "k.s")
    subprocess.check_call([hb.hipcc()] + flags + ["--cuda-device-only", "-S", "-x", "hip", src, "-o", out], stderr=subprocess.DEVNULL)
    text = open(out).read()

for blk in re.split(r"\n(?=\s*\.globl\s)", text):
    m = re.search(r"\.globl\s+(\S+)", blk)
    if not m or ".amdhsa_kernel" not in blk:
        continue
    name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", name)).split("(")[0]
    if flt and flt not in name:
        continue
    g = lambda k: (re.search(r"\." + k + r"\s+(\d+)", blk) or [None, "?"])[1]
    # LLVM annotates every basic block with the loop it belongs to ("Loop Header: Depth=1", "in Loop: Header=BB3_7 Depth=1")
    depth, loads, barrier_seen, after_barrier, in_loop, run, best = 0, 0, False, 0, 0, 0, 0
    print(f"{name}: vgpr {g('amdhsa_next_free_vgpr')} lds {g('amdhsa_group_segment_fixed_size')} scratch {g('amdhsa_private_segment_fixed_size')}")
    for l in blk.split(".amdhsa_kernel")[0].splitlines():
        l = l.strip()
        if re.match(r"(\.LBB\w+:|; %bb\.\d+:)", l):
            d = re.search(r"Loop.*Depth=(\d+)", l)
            d = int(d.group(1)) if d else 0
            for k in range(depth, d):
                print("  " * (k + 1) + "loop {")
            for k in range(depth, d, -1):
                print("  " * k + "}")
            depth = d
            continue
        if not l or l.startswith((";", ".")):
            continue
        pad, op = "  " * (depth + 1), l.split()[0]
        if op.startswith("global_load"):
            print(f"{pad}{op}")
            loads, run = loads + 1, run + 1
            best = max(best, run)
            after_barrier += barrier_seen
            in_loop += depth > 0
        elif op == "s_waitcnt" and "vmcnt" in l:
            print(pad + "s_waitcnt " + re.search(r"vmcnt\(\d+\)", l).group(0))
            run = 0
        elif op == "s_barrier":
            print(f"{pad}s_barrier")
            barrier_seen = True
    print(f"  => {loads} global_load: longest run without a vmcnt wait {best}, after the first barrier {after_barrier}, inside a loop {in_loop}")
