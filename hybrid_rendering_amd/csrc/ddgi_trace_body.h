// The body of the DDGI probe-trace kernels (ddgi.hip), one text for k_ddgi_trace<STATS, SHARED, CUTOUT> as it was, for k_ddgi_trace_emissive<SHARED, CUTOUT>
// and for k_ddgi_trace_lights<SHARED, CUTOUT>: included inside each kernel, which names STATS, SHARED, CUTOUT, EMISSIVE, LIGHTS, a, cv_gi, cv_shadow, em and lt.  Not a function: behind a call, however
// inlined, the code of the kernels that exist moves (docs/EXPERIMENTS.md, "Emissive materials"); textual inclusion leaves them bit for bit.
#ifndef HR_DDGI_TRACE_BODY
#error "ddgi_trace_body.h is the text of a kernel body: only ddgi.hip includes it, between the braces of its two kernels"
#endif
    static_assert(!(STATS && SHARED), "no statistics build of the two-level walk");
    static_assert(!(STATS && CUTOUT), "no statistics build of the cutout walks");
    __shared__ uint32_t s_stack[DDGI_TRACE_WAVES][HR_STACK_ENTRIES * 64];
    __shared__ CoopWaveOf<SHARED> s_coop[DDGI_TRACE_WAVES];   // the cooperative walks' scratch: an instantiation that walks per lane never names it
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R = a.d.rays_per_probe;
    const long long gid = (long long)blockIdx.x * (64 * DDGI_TRACE_WAVES) + threadIdx.x;
    const int probe = a.probe_begin + (int)(gid / R), ray = (int)(gid % R);
    uint32_t  rays = 0;
    HR_DIV(DivCounters dvp = {}, dvs = {};)
    const bool valid = probe < a.n_probes;
    f3 origin = mk3(0.0f, 0.0f, 0.0f), dir = mk3(0.0f, 0.0f, 1.0f);
    if (valid)
    {
        origin = probe_location(a.d, probe);
        const f3 f      = spherical_fibonacci((float)ray, (float)R);
        const float* M  = a.orientation;
        dir = normalize3(mk3((M[0] * f.x + M[3] * f.y) + M[6] * f.z, (M[1] * f.x + M[4] * f.y) + M[7] * f.z, (M[2] * f.x + M[5] * f.y) + M[8] * f.z));
        rays++;
    }
    uint32_t st_n = 0, st_t = 0;
    HitOf<SHARED> h;
    // the scene triple is spelled here, not taken from a context made before the primary ray: hoisting `tc` above this point changes the
    // code of the <true, false> statistics kernels (docs/EXPERIMENTS.md, "One trace kernel body"); keep `tc` at the hit
    if constexpr (STATS || (SHARED && !DDGI_COOP2))
    {
        // the per-lane walks (the statistics kernel, the perlane2 variant) take only the lanes with a ray.  This guard stays in the kernel:
        // behind a function that every lane enters, these kernels' code moves (docs/EXPERIMENTS.md, "One walk call per ray")
        h.prim = -1;
        if (valid)
        {
            if constexpr (STATS) h = trace_closest<true>(a.nodes, a.tris, origin, dir, 0.001f, 10000.0f, s_stack[wave], lane, nullptr, &st_n, &st_t);
            else h = trace_closest_of<SHARED, CUTOUT>(a.nodes, a.tris, a.sh.inst_shared, a.sh.cull[HR_RAY_GI], origin, dir, 0.001f, 10000.0f, s_stack[wave], lane, cv_gi);
        }
    }
    else h = trace_closest_wave<SHARED, CUTOUT>(valid, a.nodes, a.tris, a.sh, HR_RAY_GI, origin, dir, 0.001f, 10000.0f, s_stack[wave], s_coop[wave], lane, cv_gi HR_DIV(, &dvp));
    if (valid)
    {
        Rng   rng = rng_init((uint32_t)ray, (uint32_t)probe, a.num_frames);
        f3    L;
        float hit_distance = 10000.0f;
#ifdef HR_ABL_DDGI_PRIMARY_ONLY   // developer ablation (tools/ablate.sh): what does each part of the kernel cost?
        if (true) { L = mk3(h.t, h.u, h.v); hit_distance = h.t; }
        else
#endif
        if (h.prim < 0) L = a.sky.fetch(dir);
        else
        {
            const SurfaceHit s = surface_at(a.sh, h);
            const f3 Wo = neg3(dir);
            const f3 F0 = mix3(mk3(0.04f, 0.04f, 0.04f), s.albedo, s.metallic);
            const f3 c_diffuse = mix3(mul3(s.albedo, sub3(one3(), F0)), mk3(0.0f, 0.0f, 0.0f), s.metallic);
            const float r2x = next_float(rng), r2y = next_float(rng);
            TraceCtxOf<SHARED> tc = make_trace_ctx<SHARED>(a.nodes, a.tris, a.sh, s_stack[wave], lane);
            if constexpr (CUTOUT) tc.cv = cv_shadow;
            HR_DIV(if constexpr (!SHARED) tc.dv = &dvs;)
            f3 Lo = direct_lighting<STATS, CUTOUT>(tc, a.light, Wo, s.N, s.P, F0, c_diffuse, s.roughness, one3(), true, r2x, r2y, a.sky, rays);
            if (STATS) { st_n += tc.nn; st_t += tc.nt; }
            if constexpr (LIGHTS) Lo = add3(Lo, extra_lights_hard<CUTOUT>(tc, lt, Wo, s.N, s.P, F0, c_diffuse, s.roughness, one3(), rays));
#ifndef HR_ABL_DDGI_NO_IRRADIANCE
            if (a.infinite_bounces == 1)
#else
            if (false)
#endif
            {
                const f3 F   = fresnel_schlick_roughness(glsl_max(dot3(s.N, Wo), 0.0f), F0, s.roughness);
                const f3 kD  = scale3(sub3(one3(), F), 1.0f - s.metallic);
                const f3 irr = sample_irradiance(a.d, s.P, s.N, Wo, a.prev_irr, a.prev_depth);
                Lo = add3(Lo, mul3(mul3(scale3(kD, a.gi_intensity), c_diffuse), irr));
            }
            if constexpr (EMISSIVE)
            {
                f3 E;
                if (emission_at_hit(em, a.sh, h, E)) Lo = add3(Lo, E);
            }
            L = Lo;
            hit_distance = 0.001f + h.t;
        }
        const size_t o = (size_t)probe * R + ray;
#if defined(HR_TRACE_DIVERGENCE) && defined(HR_DDGI_DUMP_STEPS)   // developer study (tools/ddgi_sort_study.py): node steps of the primary ray in the unused .w
        a.radiance[o] = make_uint2(pack_h2(L.x, L.y), pack_h2(L.z, (float)dvp.lane_nodes));
#else
        a.radiance[o] = make_uint2(pack_h2(L.x, L.y), pack_h2(L.z, 0.0f));
#endif
        a.dirdist[o]  = make_uint2(pack_h2(dir.x, dir.y), pack_h2(dir.z, hit_distance));
    }
    HR_DIV(div_flush(dvp, g_div_ddgi); div_flush(dvs, g_div_ddgi + 8);)
    for (int o = 32; o > 0; o >>= 1) rays += __shfl_down(rays, o);
    if (lane == 0) a.ray_slots[blockIdx.x * DDGI_TRACE_WAVES + wave] = rays;
    if (STATS)
    {
        for (int o = 32; o > 0; o >>= 1) { st_n += __shfl_down(st_n, o); st_t += __shfl_down(st_t, o); }
        if (lane == 0) { atomicAdd(a.stats + 0, (unsigned long long)st_n); atomicAdd(a.stats + 1, (unsigned long long)st_t); atomicAdd(a.stats + 2, (unsigned long long)rays); }
    }
