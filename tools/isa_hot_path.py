"""Static instruction counts along the HOT path of kf_shadows_temporal (no GPU needed), next to tools/isa_stats.py's whole-kernel counts.

The kernel holds its pixel program twice: the first run, and a cold copy that a wave enters only when a history tap sat on a knife edge.
Whole-kernel counts are dominated by the cold copy, so this walks the control-flow graph of the gfx950 assembly from the kernel's entry and
leaves out the cold copy's entry block: the fall-through block behind the conditional branch that follows the first run's three stores
(where the centre texels are loaded again).  What it reaches is the first run — every block a wave can execute without running twice,
both sides of divergent branches included — plus the riders in front of it, which are the same in every instantiation.

    python tools/isa_hot_path.py [hybrid_rendering_amd/csrc/denoise_fast_shadows.hip] [kernel-name-filter]
"""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hybrid_rendering_amd import build as hb

src = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "hybrid_rendering_amd", "csrc", "denoise_fast_shadows.hip")
flt = sys.argv[2] if len(sys.argv) > 2 else "kf_shadows_temporal"

if src.endswith(".s"):
    text = open(src).read()
else:
    with tempfile.TemporaryDirectory() as td:
        flags = [f for f in hb.FLAGS if f not in ("-shared",)] + os.environ.get("HR_CFLAGS", "").split()
        out = os.path.join(td, "k.s")
        subprocess.check_call([hb.hipcc()] + flags + ["-x", "hip", "--cuda-device-only", "-S", src, "-o", out], stderr=subprocess.DEVNULL)
        text = open(out).read()


def blocks_of(body):
    """[(label or None, [instruction lines])] in layout order"""
    out, cur, name = [], [], None
    for line in body.splitlines():
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        if m or re.match(r"^; %bb\.\d+:", line):
            out.append((name, cur))
            cur, name = [], (m.group(1) if m else None)
            continue
        if re.match(r"^\s+[a-z]", line) and not line.strip().startswith("."):
            cur.append(line.strip())
    out.append((name, cur))
    return out


def hot_blocks(blocks):
    index = {name: i for i, (name, _) in enumerate(blocks) if name}
    # the cold copy's entry: the fall-through block behind a conditional branch that starts by loading the centre texels again
    cold = None
    for i in range(1, len(blocks)):
        prev, ins = blocks[i - 1][1], blocks[i][1]
        head = [l for l in ins if not l.startswith("s_nop")][:3]
        if prev and prev[-1].startswith("s_cbranch_") and len(head) == 3 and all(l.startswith("global_load_") for l in head):
            cold = i
            break
    assert cold is not None, "the cold copy's entry block was not found"
    reach, todo = set(), [0]
    while todo:
        i = todo.pop()
        if i in reach or i == cold or i >= len(blocks):
            continue
        reach.add(i)
        ins = blocks[i][1]
        fall = True
        for l in ins:
            op = l.split()[0]
            if op.startswith("s_cbranch_") or op == "s_branch":
                tgt = l.split()[1]
                if tgt in index:
                    todo.append(index[tgt])
                if op == "s_branch":
                    fall = False
            if op == "s_endpgm":
                fall = False
        if fall:
            todo.append(i + 1)
    return reach, cold


for blk in re.split(r"\n(?=\s*\.globl\s)", text):
    m = re.search(r"\.globl\s+(\S+)", blk)
    if not m or ".amdhsa_kernel" not in blk:
        continue
    name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
    if flt not in name:
        continue
    body = blk.split(".amdhsa_kernel")[0]
    blocks = blocks_of(body)
    reach, cold = hot_blocks(blocks)
    hot = [l.split()[0] for i in sorted(reach) for l in blocks[i][1]]
    every = [l.split()[0] for _, ins in blocks for l in ins]
    cnt = lambda ins, p: sum(1 for i in ins if re.match(p, i))
    g = lambda k: (re.search(r"\." + k + r"\s+(\d+)", blk) or [None, "?"])[1]
    short = re.sub(r"\(anonymous namespace\)::", "", name)
    short = re.sub(r"^void ", "", short).split("(")[0]
    print(f"{short[-32:]:32s} vgpr {g('amdhsa_next_free_vgpr'):>3} scratch {g('amdhsa_private_segment_fixed_size'):>3} lds {g('amdhsa_group_segment_fixed_size'):>5} | "
          f"all: valu {cnt(every, r'v_'):4d} | hot: valu {cnt(hot, r'v_'):4d} (trans {cnt(hot, r'v_(rcp|rsq|sqrt|exp|log)_'):2d}) salu {cnt(hot, r's_'):4d} "
          f"vmem {cnt(hot, r'global_'):3d} lds {cnt(hot, r'ds_'):3d} spill st {cnt(hot, r'scratch_store'):2d} ld {cnt(hot, r'scratch_load'):2d}")
