"""GPU fuzzer of the deformable scenes (csrc/deform.hip): random scenes (a heightfield, the Cornell box, a triangle soup of tests/ray_cases.py),
random sequences of synth.deform steps applied over random sub-ranges through hr_scene_update_vertices, a hr_scene_rebuild and a
hr_scene_rebuild_device (the triangles re-dealt among the standing tree's leaves by kernels, csrc/deform_redeal.hip) now and then.  After
every step queries (uniform rays, grazers of the scene's own child boxes, rays through edges and vertices) equal those of a fresh
hr_scene_create over the same vertices and the oracle's brute force, bit for bit.      python tools/fuzz_deform.py [seed] [n]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    import torch
    import ray_cases as rc
    import test_gpu_deformable as T
    from hybrid_rendering_amd import api as hr, synth
    from oracle import pyoracle
    pyoracle.build(); pyoracle.lib()
    ctx = hr.Context(0)
    rng = np.random.RandomState(seed)
    rays_total = 0
    for trial in range(n):
        pick = rng.randint(0, 3)
        if pick == 0:
            sd0 = synth.heightfield(int(rng.randint(4, 48)), seed=int(rng.randint(1 << 30)), strip=int(rng.randint(0, 12)))
        elif pick == 1:
            sd0 = synth.cornell32()
        else:
            v, _ = rc.soup_of_kind(rc.SOUP_KINDS[rng.randint(len(rc.SOUP_KINDS))], int(rng.randint(1 << 30)), max_tris=4000)
            v = np.asarray(v, np.float32).reshape(-1, 3, 3)
            v = np.ascontiguousarray(v[np.isfinite(v).all((1, 2))])   # non-finite triangles get no reference: the caller's responsibility
            sd0 = synth.SceneData(v, np.tile(np.float32([0, 1, 0]), (len(v), 3, 1)), np.zeros(len(v), np.uint32), np.ones(len(v), np.uint32), np.array([[0.5] * 3 + [0, 0.5, 0, 0, 0]], np.float32), "soup")
        g = hr.Scene(ctx, sd0, deformable=True)
        cur = sd0
        for step in range(int(rng.randint(2, 6))):
            nxt = synth.deform(sd0, int(rng.randint(0, 8)), synth.DEFORM_KINDS[rng.randint(len(synth.DEFORM_KINDS))])
            first = int(rng.randint(0, sd0.n_tris))
            count = int(rng.randint(1, sd0.n_tris - first + 1)) if rng.randint(3) else sd0.n_tris - first
            v, nr = cur.verts.copy(), cur.normals.copy()
            v[first:first + count], nr[first:first + count] = nxt.verts[first:first + count], nxt.normals[first:first + count]
            cur = synth.SceneData(v, nr, sd0.tri_material, sd0.tri_mesh_id, sd0.materials, sd0.name)
            T.update(g, cur, normals=bool(rng.randint(2)), first=first, count=count)
            if rng.randint(5) == 0:
                g.rebuild()
                assert g.refit_cost() == 1.0
            if rng.randint(4) == 0:
                g.rebuild_device()      # the next step's sub-range update goes through the re-dealt triangle -> reference map
            osc, gf = pyoracle.Scene(cur), hr.Scene(ctx, cur)
            for name, rays in T.ray_sets(g, cur.verts, int(rng.randint(1 << 30)), n_random=4000, n_boxes=40, n_tris=60).items():
                what = f"seed {seed} trial {trial} step {step} ({sd0.name}, {sd0.n_tris} triangles, range [{first}, {first + count})) {name}"
                T.assert_same(T.answers(g, T.cuda(rays)), T.answers(gf, T.cuda(rays)), what)
                T.compare_with_brute_force(g, osc, rays, what)
                rays_total += len(rays)
            T.check_boxes(g, cur, f"seed {seed} trial {trial} step {step}")
            gf.close()
        g.close()
    print(f"fuzz_deform: seed {seed}, {n} scenes, {rays_total} rays: all equal a fresh scene and brute force")


if __name__ == "__main__":
    main()
