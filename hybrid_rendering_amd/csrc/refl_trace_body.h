// The body of the reflection trace kernels (reflections.hip), one text for k_refl_trace<STATS, SHARED, CUTOUT> as it was and for
// k_refl_trace_emissive<SHARED, CUTOUT> and k_refl_trace_lights<SHARED, CUTOUT>: included inside each kernel, which names STATS, SHARED, CUTOUT, EMISSIVE,
// LIGHTS, a, cv_refl, cv_shadow, em and lt
// (see ddgi_trace_body.h for why this is not a function).
#ifndef HR_REFL_TRACE_BODY
#error "refl_trace_body.h is the text of a kernel body: only reflections.hip includes it, between the braces of its two kernels"
#endif
    static_assert(!(STATS && SHARED), "no statistics build of the two-level walk");
    static_assert(!(STATS && CUTOUT), "no statistics build of the cutout walks");
    __shared__ uint32_t s_stack[REFL_TRACE_WAVES][HR_STACK_ENTRIES * 64];
    __shared__ CoopWaveOf<SHARED> s_coop[REFL_TRACE_WAVES];   // the cooperative walks' scratch: an instantiation that walks per lane never names it
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int launch_slot = blockIdx.x * REFL_TRACE_WAVES + wave;
    if (launch_slot >= a.tiles_x * a.tiles_y) return;   // wave-uniform
    const int tile = a.order ? (int)a.order[launch_slot] : launch_slot;
    const unsigned long long t_begin = a.cost ? wall_clock64() : 0ull;
    const int x = (tile % a.tiles_x) * 8 + (lane & 7), y = (tile / a.tiles_x + a.tile_y0) * 8 + (lane >> 3);
    uint32_t  rays = 0;
    HR_DIV(DivCounters dvp = {}, dvs = {};)
    // per pixel: the reflection ray (or none); the wave stays converged around the traversal
    const size_t o = (size_t)y * a.w + x;
    bool  geom = false, trace = false;
    f3    color = mk3(0.0f, 0.0f, 0.0f), dir = mk3(0.0f, 0.0f, 1.0f), ray_origin = mk3(0.0f, 0.0f, 0.0f);
    float ray_length = -1.0f;
    // the lane's DDGI gather, if any (kind 1: rough pixel, 2: hit point) and what its result is combined with
    int gather = 0;
    f3  gP = mk3(0.0f, 0.0f, 0.0f), gN = mk3(0.0f, 0.0f, 1.0f), gWo = mk3(0.0f, 0.0f, 1.0f);
    f3  hLo = mk3(0.0f, 0.0f, 0.0f), hkD = hLo, hcd = hLo, hspec = hLo;
    [[maybe_unused]] f3   hE = mk3(0.0f, 0.0f, 0.0f);   // EMISSIVE: the hit's emission, added after the gather
    [[maybe_unused]] bool emits = false;
    if (x < a.w && y >= a.y0 && y < a.y1)
    {
        const float  dp = a.depth[o];
        if (dp == 1.0f) a.out[o] = make_uint2(0u, pack_h2(0.0f, -1.0f));
        else
        {
            geom = true;
            const uint2 g2 = a.gb2[o], g3 = a.gb3[o];
            const float roughness = h2f_lo(g3.x);
            const float tu = __fdiv_rn((float)x + 0.5f, (float)a.w), tv = __fdiv_rn((float)y + 0.5f, (float)a.h);
            const f3 P  = world_pos_from_depth(tu, tv, dp, a.vpi);
            const f3 N  = oct_decode(h2f_lo(g2.x), h2f_hi(g2.x));
            const f3 Wo = normalize3(sub3(mk3(a.cam[0], a.cam[1], a.cam[2]), P));
            ray_origin  = add3(P, scale3(N, a.bias));
            if (roughness < 0.05f) { dir = reflect3(neg3(Wo), N); trace = true; }
            else if (roughness > 0.75f && a.approximate_with_ddgi == 1)
            {
                gather = 1; gP = P; gN = reflect3(neg3(Wo), N); gWo = Wo;
            }
            else
            {
                const float r0 = sample_blue_noise(x, y, (int)a.num_frames, 0, a.sobol, a.sr) * a.trim;
                const float r1 = sample_blue_noise(x, y, (int)a.num_frames, 1, a.sobol, a.sr) * a.trim;
                const f3    Wh = importance_sample_ggx(r0, r1, N, roughness);
                dir   = reflect3(neg3(Wo), Wh);
                trace = true;
            }
        }
    }
    if (trace) rays++;
    uint32_t st_n = 0, st_t = 0;
    HitOf<SHARED> hit;
    // the scene triple is spelled here, not taken from a context made before the primary ray: hoisting `tc` above this point changes the
    // code of the <true, false> statistics kernels (docs/EXPERIMENTS.md, "One trace kernel body"); keep `tc` at the hit
    if constexpr (STATS || (SHARED && !REFL_COOP2))
    {
        // the per-lane walks take only the lanes with a ray; the guard stays in the kernel (see k_ddgi_trace)
        hit.prim = -1;
        if (trace)
        {
            if constexpr (STATS) hit = trace_closest<true>(a.nodes, a.tris, ray_origin, dir, 0.001f, 10000.0f, s_stack[wave], lane, nullptr, &st_n, &st_t);
            else hit = trace_closest_of<SHARED, CUTOUT>(a.nodes, a.tris, a.sh.inst_shared, a.sh.cull[HR_RAY_REFLECTION], ray_origin, dir, 0.001f, 10000.0f, s_stack[wave], lane, cv_refl);
        }
    }
    else hit = trace_closest_wave<SHARED, CUTOUT>(trace, a.nodes, a.tris, a.sh, HR_RAY_REFLECTION, ray_origin, dir, 0.001f, 10000.0f, s_stack[wave], s_coop[wave], lane, cv_refl HR_DIV(, &dvp));
    if (trace)
    {
        if (hit.prim < 0) { color = a.env.sky.fetch(dir); ray_length = -1.0f; }
        else
        {
            const SurfaceHit s = surface_at(a.sh, hit);
            const f3 hWo = neg3(dir);
            const f3 F0  = mix3(mk3(0.04f, 0.04f, 0.04f), s.albedo, s.metallic);
            const f3 c_diffuse = mix3(mul3(s.albedo, sub3(one3(), F0)), mk3(0.0f, 0.0f, 0.0f), s.metallic);
            TraceCtxOf<SHARED> tc = make_trace_ctx<SHARED>(a.nodes, a.tris, a.sh, s_stack[wave], lane);
            if constexpr (CUTOUT) tc.cv = cv_shadow;
            HR_DIV(if constexpr (!SHARED) tc.dv = &dvs;)
            CubeMap  none { nullptr, 0 };
            hLo = direct_lighting<STATS, CUTOUT>(tc, a.light, hWo, s.N, s.P, F0, c_diffuse, s.roughness, one3(), false, 0.0f, 0.0f, none, rays);
            if (STATS) { st_n += tc.nn; st_t += tc.nt; }
            if constexpr (LIGHTS) hLo = add3(hLo, extra_lights_hard<CUTOUT>(tc, lt, hWo, s.N, s.P, F0, c_diffuse, s.roughness, one3(), rays));
            if (a.sample_gi == 1)
            {
                const f3    R   = reflect3(neg3(hWo), s.N);
                const float ndv = glsl_max(dot3(s.N, hWo), 0.0f);
                const f3    F   = fresnel_schlick_roughness(ndv, F0, s.roughness);
                hkD             = scale3(sub3(one3(), F), 1.0f - s.metallic);
                const f3    pre = a.env.prefiltered_fetch(R, s.roughness * 4.0f);
                float bx, by;
                a.env.lut_fetch(ndv, s.roughness, bx, by);
                hspec = scale3(mul3(pre, add3(scale3(F, bx), mk3(by, by, by))), a.ibl_intensity);
                hcd   = c_diffuse;
                gather = 2; gP = s.P; gN = s.N; gWo = hWo;
            }
            if constexpr (EMISSIVE) emits = emission_at_hit(em, a.sh, hit, hE);
            color      = hLo;
            ray_length = 0.001f + hit.t;
        }
    }
    // ONE parity gather for the rough pixels and the hit points of the tile (shading.h; the traversal stack is idle here — the cooperative A/B form borrows it)
    {
        const f3 net = sample_irradiance_net_coop(gather != 0, a.d, gP, gN, gWo, a.irr, a.dep, reinterpret_cast<float*>(s_stack[wave]), lane);
        if (gather == 1) color = scale3(irradiance_from_net(a.d, net), a.rough_ddgi_intensity);
        else if (gather == 2)
        {
            const f3 diffuse = mul3(scale3(hcd, a.gi_intensity), irradiance_from_net(a.d, net));
            color = add3(hLo, add3(mul3(hkD, diffuse), hspec));
        }
    }
    if constexpr (EMISSIVE)
        if (emits) color = add3(color, hE);   // a hit lane: color is the gather's sum (gather == 2) or hLo
    if (geom) a.out[o] = make_uint2(pack_h2(glsl_min(color.x, 0.7f), glsl_min(color.y, 0.7f)), pack_h2(glsl_min(color.z, 0.7f), ray_length));
    HR_DIV(div_flush(dvp, g_div_refl); div_flush(dvs, g_div_refl + 8);)
    for (int o2 = 32; o2 > 0; o2 >>= 1) rays += __shfl_down(rays, o2);
    if (lane == 0) a.ray_slots[tile] = rays;
    if (lane == 0 && a.cost)
    {
        const unsigned long long ticks = wall_clock64() - t_begin;
        a.cost[tile] = (uint16_t)(ticks > 65535ull ? 65535ull : ticks);
    }
    if (STATS)
    {
        for (int o2 = 32; o2 > 0; o2 >>= 1) { st_n += __shfl_down(st_n, o2); st_t += __shfl_down(st_t, o2); }
        if (lane == 0) { atomicAdd(a.stats + 0, (unsigned long long)st_n); atomicAdd(a.stats + 1, (unsigned long long)st_t); atomicAdd(a.stats + 2, (unsigned long long)rays); }
    }
