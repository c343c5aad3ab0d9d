// The body of the ground-truth path-trace kernels (ground_truth.hip), one text for k_ground_truth<INDIRECT, SHARED, CUTOUT> as it was and for
// k_ground_truth_emissive<INDIRECT, SHARED, CUTOUT> and k_ground_truth_lights<INDIRECT, SHARED, CUTOUT>: included inside each kernel, which names INDIRECT,
// SHARED, CUTOUT, EMISSIVE, LIGHTS, a, cv_primary, cv_gi, cv_shadow, em and lt (see ddgi_trace_body.h for why this is not a function).
#ifndef HR_GROUND_TRUTH_BODY
#error "ground_truth_body.h is the text of a kernel body: only ground_truth.hip includes it, between the braces of its two kernels"
#endif
    __shared__ uint32_t s_stack[HR_STACK_ENTRIES * 64];
    const int lane = threadIdx.x;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x + a.tile_y0;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    uint32_t  rays = 0;
    if (x < a.w && y >= a.y0 && y < a.y1)
    {
        Rng rng = rng_init((uint32_t)x, (uint32_t)y, a.num_frames);
        const float jx = next_float(rng), jy = next_float(rng);
        const float px = ((float)x + 0.5f) + jx, py = ((float)y + 0.5f) + jy;
        const float tcx = __fdiv_rn(px, (float)a.w) * 2.0f - 1.0f, tcy = __fdiv_rn(py, (float)a.h) * 2.0f - 1.0f;
        const f4 origin = mul_m4(a.view_inverse, 0.0f, 0.0f, 0.0f, 1.0f);
        const f4 target = mul_m4(a.proj_inverse, tcx, tcy, 1.0f, 1.0f);
        const f3 tn     = normalize3(mk3(target.x, target.y, target.z));
        const f4 dir4   = mul_m4(a.view_inverse, tn.x, tn.y, tn.z, 0.0f);
        // The payload chain of the recursive shader, unrolled.  Every nested invocation starts with L = 0 and its L is ADDED to
        // its caller's (p_Payload.L += indirect_lighting()), innermost first: adds[k] is what invocation k adds.  With
        // trace_indirect = 0 (the reference as shipped: the recursive traceRayEXT of rchit:95-105 is commented out) the loop
        // runs once.  trace_indirect = 1 re-enables that call (SURVEY 8f row 3's optional extension), rchit:67-108 verbatim.
        f3       o = mk3(origin.x, origin.y, origin.z), d = mk3(dir4.x, dir4.y, dir4.z);
        f3       T = one3();
        float    t_min = 0.001f;
        f3       adds[INDIRECT ? GT_MAX_DEPTH : 1];
        int      depth = 0;
        uint32_t nn = 0, nt = 0;
        TraceCtxOf<SHARED> tc = make_trace_ctx<SHARED>(a.nodes, a.tris, a.sh, s_stack, lane);
        if constexpr (CUTOUT) tc.cv = cv_shadow;
        for (;; depth++)
        {
            adds[depth] = mk3(0.0f, 0.0f, 0.0f);
            rays++;
            // the camera ray, then the bounces: their own ray classes (tc's is the visibility rays').  The view and the cull mask are picked only
            // where they are read: picking them in every instantiation changes the code of the INDIRECT kernels (docs/EXPERIMENTS.md, "One walk call per ray")
            CutoutView cv;
            if constexpr (CUTOUT) cv = depth == 0 ? cv_primary : cv_gi;
            HitOf<SHARED> h;
            h = trace_closest_of<SHARED, CUTOUT>(a.nodes, a.tris, a.sh.inst_shared, SHARED ? a.sh.cull[depth == 0 ? HR_RAY_PRIMARY : HR_RAY_GI] : 0u, o, d, t_min, 10000.0f, s_stack, lane, cv);
            if (h.prim < 0)
            {
                const f3 env = a.sky.fetch(d);
                adds[depth]  = depth == 0 ? env : mul3(T, env);   // rmiss:26-34
                break;
            }
            SurfaceHit s = surface_at(a.sh, h);
            s.N = normalize3(s.N);   // rchit:131 normalises fetch_normal()'s result once more (observable with normal maps)
            const float roughness = s.roughness * a.roughness_multiplier;
            const f3 Wo = neg3(d);
            const f3 F0 = mix3(mk3(0.04f, 0.04f, 0.04f), s.albedo, s.metallic);
            const f3 c_diffuse = mix3(mul3(s.albedo, sub3(one3(), F0)), mk3(0.0f, 0.0f, 0.0f), s.metallic);
            const float r1x = next_float(rng), r1y = next_float(rng), r2x = next_float(rng), r2y = next_float(rng);
            f3       Lo = mk3(0.0f, 0.0f, 0.0f);
            const f3 ray_origin = add3(s.P, scale3(s.N, 0.1f));
            {
                f3    Wi;
                float t_max, attenuation;
                fetch_light_shadow(a.light, s.P, s.N, r1x, r1y, Wi, t_max, attenuation);
                const f3 Li = scale3(mk3(a.light.data2[0], a.light.data2[1], a.light.data2[2]), a.light.data0[3]);
                const f3 Wh = normalize3(add3(Wo, Wi));
                if (attenuation > 0.0f)
                {
                    rays++;
                    attenuation = attenuation * (visibility_ray_occluded<false, CUTOUT>(tc, ray_origin, Wi, 0.01f, t_max, nn, nt) ? 0.0f : 1.0f);
                }
                const f3 brdf = evaluate_uber_brdf(c_diffuse, roughness, s.N, F0, Wo, Wh, Wi);
                Lo = add3(Lo, mul3(scale3(mul3(T, brdf), attenuation), Li));
            }
            {
                const f3 Wi = sample_cosine_lobe_n(s.N, r2x, r2y);
                f3       Li = a.sky.fetch(Wi);
                const f3 Wh = normalize3(add3(Wo, Wi));
                rays++;
                Li = scale3(Li, visibility_ray_occluded<false, CUTOUT>(tc, ray_origin, Wi, 0.01f, 10000.0f, nn, nt) ? 0.0f : 1.0f);
                const f3 brdf = evaluate_uber_brdf(c_diffuse, roughness, s.N, F0, Wo, Wh, Wi);
                Lo = add3(Lo, mul3(mul3(T, brdf), Li));
            }
            if constexpr (LIGHTS) Lo = add3(Lo, extra_lights_soft<CUTOUT>(tc, lt, Wo, s.N, s.P, ray_origin, F0, c_diffuse, roughness, T, r1x, r1y, rays));
            if constexpr (EMISSIVE)
            {
                f3 E;
                if (emission_at_hit(em, a.sh, h, E)) Lo = add3(Lo, depth == 0 ? E : mul3(T, E));
            }
            adds[depth] = Lo;
            if (!INDIRECT || !((uint32_t)(depth + 1) < a.max_ray_bounces) || depth + 1 >= GT_MAX_DEPTH - 1) break;
            // indirect_lighting (rchit:67-108); sample_uber_brdf takes the RNG BY VALUE (brdf.glsl:146): the lobe sample re-uses
            // the numbers the Russian roulette and the next bounce draw
            Rng copy = rng;
            const float rvx = next_float(copy), rvy = next_float(copy), rvz = next_float(copy);
            const float alpha = roughness * roughness;
            f3 Wi, Wh;
            if (rvx < 0.5f)
            {
                Wh = sample_specular_ggx_lobe(s.N, alpha, rvy, rvz);
                const f3 I = neg3(Wo);
                Wi = roughness < 0.05f ? sub3(I, scale3(s.N, 2.0f * dot3(s.N, I))) : sub3(I, scale3(Wh, 2.0f * dot3(Wh, I)));
            }
            else
            {
                Wi = sample_cosine_lobe_n(s.N, rvy, rvz);
                Wh = normalize3(add3(Wo, Wi));
            }
            const float NdotL = glsl_max(dot3(s.N, Wi), 0.0f), NdotH = glsl_max(dot3(s.N, Wh), 0.0f), VdotH = glsl_max(dot3(Wi, Wh), 0.0f);
            const float pd  = __fdiv_rn(NdotL, HR_M_PI);
            const float ps  = __fdiv_rn(D_ggx(NdotH, alpha) * NdotH, glsl_max(HR_EPSILON, 4.0f * VdotH));
            const float pdf = mix1(pd, ps, 0.5f);
            const f3    brdf = evaluate_uber_brdf(c_diffuse, roughness, s.N, F0, Wo, Wh, Wi);
            const float cos_theta = glsl_clamp(dot3(s.N, Wi), 0.0f, 1.0f);
            const f3    tb = mul3(T, scale3(brdf, cos_theta));
            f3 Tn = mk3(__fdiv_rn(tb.x, pdf), __fdiv_rn(tb.y, pdf), __fdiv_rn(tb.z, pdf));
            const float probability = glsl_max(Tn.x, glsl_max(Tn.y, Tn.z));
            if (next_float(rng) > probability) break;
            Tn = scale3(Tn, __fdiv_rn(1.0f, probability));
            T = Tn; o = s.P; d = Wi; t_min = 0.0001f;
        }
        f3 L = adds[depth];
        for (int k = depth - 1; k >= 0; k--) L = add3(adds[k], L);
        const f3 clamped = mk3(glsl_min(L.x, 1.0f), glsl_min(L.y, 1.0f), glsl_min(L.z, 1.0f)); // RADIANCE_CLAMP_COLOR
        f3 out = clamped;
        const size_t i = (size_t)y * a.w + x;
        if (a.num_frames != 0u)
        {
            const uint2 q  = a.prev[i];
            const f3    pc = mk3(h2f_lo(q.x), h2f_hi(q.x), h2f_lo(q.y));
            const float n  = (float)a.num_frames;
            out = mk3(pc.x + __fdiv_rn(clamped.x - pc.x, n), pc.y + __fdiv_rn(clamped.y - pc.y, n), pc.z + __fdiv_rn(clamped.z - pc.z, n));
        }
        a.cur[i] = make_uint2(pack_h2(out.x, out.y), pack_h2(out.z, 1.0f));
    }
    for (int o = 32; o > 0; o >>= 1) rays += __shfl_down(rays, o);
    if (lane == 0) a.ray_slots[blockIdx.x] = rays;
