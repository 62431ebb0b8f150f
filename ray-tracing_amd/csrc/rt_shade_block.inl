/* rt_shade_block.inl — the rest of one iteration of Trace's bounce loop (RC:488-538) for a lane whose intersection `h` is complete: the
 * one statement of the results contract's shade rules (draw order, RC:499-538).  Textually included by rt_shade_phase.inl (the frame,
 * cost and rt_radiance kernels) and by rt_radiance_nee_kernel (rt_kernels.h).  Not a header: it reads and writes the including
 * function's locals (a, h, rng, rpos, rdir, transmittance, pathLight, bounce, extBase, st, endPath; STATS, MANY, SKY_SUN), and sets endPath
 * where the path ends; what an ended path does is the including site's.
 * Three hooks, one per amendment of include/rt_nee.h, defined by the including site and undefined right after the include (macros: a
 * callable changed the register allocation of the > 64-model trace kernel):
 *   RT_SHADE_EMIT(e)        the emission add of the opaque branch, e = emitted * transmittance
 *   RT_SHADE_OPAQUE_END     the end of the opaque branch (isSpecular, lerpT in scope)
 *   RT_SHADE_NEXT_RAY       behind the next segment's rpos / rdir, before the roulette draw (hpos, normal in scope) */
            if (h.obj < 0) {
                phase_mark<STATS>(st, PH_SKY);
                const RT_CAS KArgs& c = cold_args();
                const int32_t useSky = c.useSky; /* bit 0: UseSky; bit 1: the launch's sun is never seen (rt_sky.h; frame and cost launches only) */
                if (useSky) {
                    if constexpr (SKY_SUN) pathLight = pathLight + transmittance * environment_light_frame<STATS>(c, useSky, rdir, st);
                    else pathLight = pathLight + transmittance * environment_light(c, rdir);
                }
                endPath = true;
            } else {
                /* resolve the winner: position, normal, material */
                phase_mark<STATS>(st, PH_SHADE_HIT);
                rt_f3 hpos, normal;
                resolve_hit(a, rpos, rdir, h, hpos, normal);
                const DMaterial mat = a.materials[h.obj];

                /* The glass (RC:499-518) and opaque (RC:519-533) branches both draw
                 * diffuseDir = normalize(normal + RandomDirection) — the costliest piece
                 * (3 log, 3 cos, 4 sqrt).  It is hoisted so that all hit lanes execute it
                 * together; each lane still consumes its random numbers in its branch's
                 * order: opaque = [isSpecular, direction x6], glass = [direction x6, choice]. */
                const bool isGlass = mat.flag == RT_MATERIAL_GLASS;
                float uSpec = 0.0f;
                if (!isGlass) uSpec = rt_random_value(&rng); /* RC:521 */
                const rt_f3 diffuseDir = rt_normalize(normal + rand_direction(&rng)); /* RC:509 / RC:525 */
                /* Both branches end in normalize(lerp(A, B, t)) of a direction pair: opaque (diffuseDir, reflect, smoothness x
                 * isSpecular), glass either (diffuseDir, reflect, specularProbability) or (-diffuseDir, refract, smoothness).  The
                 * reference normalises both glass candidates and keeps one (RC:511-516); only the kept one is observable, so the
                 * branches just pick (A, B, t) and ONE lerp + normalize follows for all hit lanes. */
                const rt_f3 specularDir = rt_reflect(rdir, normal); /* == the glass branch's reflectDir, RC:419-422 */
                rt_f3 lerpA = diffuseDir, lerpB = specularDir;
                float lerpT;
                if (isGlass) {
                    phase_mark<STATS>(st, PH_GLASS);
                    if (h.backface) { /* RC:502 */
                        rt_f3 e = ((-h.dst) * rt_v3(mat.absorption[0], mat.absorption[1], mat.absorption[2])) * mat.absorptionStrength;
                        transmittance = transmittance * rt_v3(rtd_exp(e.x), rtd_exp(e.y), rtd_exp(e.z));
                    }
                    float iorCurrent = h.backface ? mat.ior : 1.0f;
                    float iorNext = h.backface ? 1.0f : mat.ior;
                    const rt_f3 refractDir = refract_dir(rdir, normal, iorCurrent, iorNext);
                    const float reflectWeight = reflectance(rdir, normal, iorCurrent, iorNext);
                    const bool followReflection = rt_random_value(&rng) <= reflectWeight; /* RC:515 */
                    lerpT = mat.specularProbability;
                    if (!followReflection) {
                        lerpA = -diffuseDir;
                        lerpB = refractDir;
                        lerpT = mat.smoothness;
                    }
                } else {
                    const bool isSpecular = mat.specularProbability >= uSpec;
                    lerpT = mat.smoothness * (isSpecular ? 1.0f : 0.0f);
                    rt_f3 emitted = rt_v3(mat.emissionCol[0], mat.emissionCol[1], mat.emissionCol[2]) * mat.emissionStrength;
                    RT_SHADE_EMIT(emitted * transmittance);
                    transmittance = transmittance * material_colour(mat, hpos, normal, isSpecular);
                    RT_SHADE_OPAQUE_END
                }
                rdir = rt_normalize(rt_lerp3(lerpA, lerpB, lerpT));
                rpos = isGlass ? hpos + (0.001f * normal) * rt_sign(rt_dot(normal, rdir)) : hpos + (normal * 0.001f);
                RT_SHADE_NEXT_RAY
                /* RC:535-538 Russian roulette */
                float p = rt_max(transmittance.x, rt_max(transmittance.y, transmittance.z));
                if (rt_random_value(&rng) >= p) {
                    endPath = true;
                } else {
                    transmittance = transmittance * rt_rcp(p);
                    if (MANY) {
                        const uint32_t b = extBase[(1 + a.extWords) * RT_WAVE] + 1u;
                        extBase[(1 + a.extWords) * RT_WAVE] = b;
                        if ((int)b > a.maxBounce) endPath = true;
                    } else {
                        bounce++;
                        if (bounce > a.maxBounce) endPath = true; /* RC:485: i <= MaxBounceCount */
                    }
                }
            }
