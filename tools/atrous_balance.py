"""How the live workgroups of the shadow pass's tolerance-mode a-trous launches spread over the CUs (HR_DEBUG_ATROUS_TIMELINE): per launch
(kf_shadows_atrous01, kf_shadows_atrous<4>, kf_shadows_atrous<8>) the live units (the workgroups that hold a tile which is no shadow tile
and so do all the work) per CU (min / mean / max, histogram) and per CU the span from its first entry to its last exit, on the bench
frame (bench.py's scene, camera ring and frame cycle).
python tools/atrous_balance.py [W H]      HR_ATROUS01_RESIDENT=<R> in the environment: the residency cap under test (0: none)"""
import os, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from hybrid_rendering_amd import api as hr, synth

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1920, 1080)
FRAMES = int(os.environ.get('ATROUS_BALANCE_FRAMES', '12'))
sd = synth.sponza_like(1.0); ctx = hr.Context(0); sc = hr.Scene(ctx, sd)
light = synth.sponza_light()
sob, sr = synth.blue_noise_tables()
sob_d, sr_d = torch.from_numpy(sob).cuda(), torch.from_numpy(sr).cuda()
R = 8
cams = [synth.sponza_camera(W / H, frame=f, dolly=0.5) for f in range(R + 1)]
ubos = [synth.make_ubo(cams[i], cams[i - 1 if i > 0 else 0], light) for i in range(R)]
gbs = [sc.gbuffer(u, W, H) for u in ubos]
torch.cuda.synchronize()
prefix = os.path.join(tempfile.mkdtemp(), 'atrous_timeline')
# the library reads its developer switches when a pass object is created (never in render)
os.environ['HR_DEBUG_ATROUS_TIMELINE'] = prefix
p = hr.RayTracedShadows(ctx, W, H)
del os.environ['HR_DEBUG_ATROUS_TIMELINE']
p.params.exact = 0
# every frame rewrites the files: the last one stands (history and the occluder cache have settled by then)
for k in range(1, FRAMES + 1):
    i, j = k % R, (k - 1) % R
    fi = hr.frame_inputs(gbs[i], gbs[j], ubos[i], k, k & 1, sob_d, sr_d)
    p.render(sc, fi)
torch.cuda.synchronize()
tiles = p.image(hr.RayTracedShadows.IMG_TILES).cpu().numpy()
print('%d x %d, frame %d: %d of %d tiles live; %s' % (W, H, FRAMES, int((tiles != 0).sum()), tiles.size,
      'HR_ATROUS01_RESIDENT=%s' % os.environ.get('HR_ATROUS01_RESIDENT', '(default)')))
p.close()

for tag in ('atrous01', 'atrous4', 'atrous8'):
    path = prefix + '.' + tag
    if not os.path.exists(path):
        print(tag, ': no record (launch not taken)'); continue
    t = np.fromfile(path, dtype=np.uint64).reshape(-1, 4)
    wg_of = np.arange(len(t)) // 4                 # four waves per workgroup, in launch order
    m = t[:, 0] != 0                               # waves that ran
    t, wg_of = t[m], wg_of[m]
    t0 = t[:, 0].min()
    start = (t[:, 0] - t0).astype(np.float64) * 0.01   # us (100 MHz)
    end = (t[:, 1] - t0).astype(np.float64) * 0.01
    hw = (t[:, 2] & 0xffffffff).astype(np.uint32); xcc = ((t[:, 2] >> 32) & 0xf).astype(np.uint32)
    cu = xcc * 1000 + ((hw >> 13) & 7) * 100 + ((hw >> 12) & 1) * 50 + ((hw >> 8) & 0xf)
    n_live = t[:, 3].astype(np.int64)             # units with a live tile the workgroup walked (0 or 1 unless the launch is strided)
    # per workgroup: its first wave's entry, its last wave's exit (the waves of a workgroup share a CU)
    wgs, first = np.unique(wg_of, return_index=True)
    w_start = np.minimum.reduceat(start, first); w_end = np.maximum.reduceat(end, first)
    w_cu, w_v = cu[first], n_live[first]
    live, dead = w_v >= 1, w_v == 0
    cus = np.unique(cu)
    per_cu = np.array([w_v[w_cu == c].sum() for c in cus])
    span = np.array([w_end[w_cu == c].max() - w_start[w_cu == c].min() for c in cus])
    live_span = np.array([(w_end[live & (w_cu == c)].max() - w_start[live & (w_cu == c)].min()) if (live & (w_cu == c)).any() else 0.0 for c in cus])
    print('%s: launch span %.1f us; workgroups %d, with a live unit %d, without %d; live units %d; CUs seen %d' % (
        tag, w_end.max(), len(wgs), live.sum(), dead.sum(), w_v.sum(), len(cus)))
    print('  live units per CU: min %d  mean %.2f  max %d' % (per_cu.min(), per_cu.mean(), per_cu.max()))
    print('  histogram (live units per CU: CUs): ' + '  '.join('%d: %d' % (k, c) for k, c in enumerate(np.bincount(per_cu)) if c))
    print('  per-CU span first entry -> last exit (us): min %.1f  mean %.1f  max %.1f;  over its live workgroups only: min %.1f  mean %.1f  max %.1f' % (
        span.min(), span.mean(), span.max(), live_span.min(), live_span.mean(), live_span.max()))
    for k in sorted(set(per_cu)):
        print('    CUs with %2d live: %3d, live span mean %.1f us' % (k, (per_cu == k).sum(), live_span[per_cu == k].mean()))
    d = w_end[live] - w_start[live]
    print('  live workgroup duration us: mean %.2f  p50 %.2f  p90 %.2f  max %.2f;  last live entry %.1f us, last live exit %.1f us' % (
        d.mean(), np.percentile(d, 50), np.percentile(d, 90), d.max(), w_start[live].max(), w_end[live].max()))
    if dead.any():
        print('  dead workgroups: last entry %.1f us, last exit %.1f us (tail behind the last live exit %.1f us)' % (
            w_start[dead].max(), w_end[dead].max(), max(0.0, w_end[dead].max() - w_end[live].max())))
