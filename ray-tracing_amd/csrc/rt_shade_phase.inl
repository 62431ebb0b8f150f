/* rt_shade_phase.inl — the second half of a wave iteration of trace_body (rt_kernels.h): the rest of one iteration of Trace's bounce loop
 * (RC:488-538) for the lanes whose intersection is complete.  Textually included at the two places it can follow the first half: directly
 * (every variant but the pooled FLAT one — the code is then exactly the nested block of rounds 1-5, a callable changed the register
 * allocation of the > 64-model variant), or behind the chain exchange that the pooled FLAT variant runs between the halves with every
 * lane of the wave present; and a third time by rt_radiance_kernel.  Not a header: it reads and writes trace_body's locals.
 * What is here is the frame's part: the test that the walk is complete, the COST snapshot, and the pixel's sum that an ended path is
 * added to.  The shade arithmetic between them is rt_shade_block.inl, included with its three hooks at their defaults. */
        if (inTrav && (FLAT || traverse<STATS, true, MANY, HOT>(a, rpos, rdir, stackBase, extBase, h, t, st, hotLds, hotUnits))) {
            inTrav = false;
            if constexpr (COST) { /* a camera ray's first segment is complete (bounce 0): close its primary snapshot; camera ray 0's outcome */
                if ((MANY ? extBase[(1 + a.extWords) * RT_WAVE] : (uint32_t)bounce) == 0u) {
                    uint4* const o = RT_COST_SLOT(cold_args()) + 1;
                    uint4 p = *o;
                    p.x += st.inner; p.y += st.leaf; p.z += st.tri;
                    if (PXU(PX_SAMPLE) == 1u) p.w = h.obj < 0 ? 0u : (a.materials[h.obj].flag == RT_MATERIAL_GLASS ? 2u : 1u);
                    *o = p;
                }
            }
            /* the rest of one iteration of Trace's bounce loop — RC:488-538 */
            bool endPath = false;
#define RT_SHADE_EMIT(e) pathLight = pathLight + (e)
#define RT_SHADE_OPAQUE_END
#define RT_SHADE_NEXT_RAY
#include "rt_shade_block.inl"
#undef RT_SHADE_EMIT
#undef RT_SHADE_OPAQUE_END
#undef RT_SHADE_NEXT_RAY
            if (endPath) {
                PXF(PX_TIX) = PXF(PX_TIX) + pathLight.x; /* RC:578: totalIncomingLight += Trace(...) */
                PXF(PX_TIY) = PXF(PX_TIY) + pathLight.y;
                PXF(PX_TIZ) = PXF(PX_TIZ) + pathLight.z;
                pathActive = false;
            }
        
        }
