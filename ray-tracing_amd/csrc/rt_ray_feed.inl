/* rt_ray_feed.inl — the head of a wave iteration of rt_radiance_kernel and rt_radiance_nee_kernel (rt_kernels.h): hand rays to the
 * lanes without a path.  Every lane of the wave is active here.  A lane without a path takes the next unassigned ray of the wave's block
 * by ballot and prefix rank; when the block is used up the wave takes another from the block counter (rt_radiance_kernel's comment).  A
 * ray that Trace would not loop for (maxBounce < 0) gets its record here and starts no path.  Declares `idle`, the ballot of the lanes
 * still without a path: all of them = no lane holds a path and there is no ray left.
 * Not a header: it reads and writes the including kernel's locals — its own state (blocks, poolBase, poolPos, queueEmpty), the path
 * (pathActive, rng, rpos, rdir, transmittance, pathLight, bounce, extBase) and a, rays, n, out, lane, MANY.  A textual include, and the
 * state plain locals, because that is the form the compiler's output chose: a function over a state struct with a start callable
 * changed all three rt_radiance_kernel bodies (+72, +40 and +122 instructions), and so does reading the arguments any other way than
 * each kernel did — hence three hooks, defined by the including site and undefined right after the include:
 *   RT_FEED_ROUND       at the top of every round of the loop (rt_radiance_kernel binds its cold_args() here)
 *   RT_FEED_ARGS        the KArgs the block counter (tileQueue) and maxBounce are read from
 *   RT_FEED_START(i)    the kernel's own part of starting ray i on the lane */
        unsigned long long idle = __ballot(!pathActive);
        while (idle) {
            RT_FEED_ROUND
            if (poolPos >= 64) {
                if (queueEmpty) break;
                int next = 0;
                if (lane == 0) next = (int)atomicAdd(RT_FEED_ARGS.tileQueue, 1ull);
                next = __builtin_amdgcn_readfirstlane(next) + (int)gridDim.x;
                if (next >= blocks) { queueEmpty = true; break; }
                poolBase = next * RT_WAVE;
                poolPos = 0;
            }
            const int rank = __popcll(idle & ((1ull << lane) - 1ull));
            const int avail = 64 - poolPos;
            if (!pathActive && rank < avail) {
                const int i = poolBase + poolPos + rank;
                if (i < n) { /* inside the n * 32 and n * 16 bytes the host checked */
                    const float4 r0 = rays[2 * (size_t)i], r1 = rays[2 * (size_t)i + 1];
                    if (RT_FEED_ARGS.maxBounce >= 0) { /* RC:485: the loop runs for i = 0 */
                        rpos = rt_v3(r0.x, r0.y, r0.z);
                        rdir = rt_v3(r1.x, r1.y, r1.z);
                        rng = __float_as_uint(r1.w);
                        transmittance = rt_v3s(1.0f);
                        pathLight = rt_v3s(0.0f);
                        if (MANY) extBase[(1 + a.extWords) * RT_WAVE] = 0u; /* (trace_body: this variant keeps the bounce count in LDS) */
                        else bounce = 0;
                        RT_FEED_START(i)
                        pathActive = true;
                    } else {
                        out[i] = make_float4(0.0f, 0.0f, 0.0f, r1.w); /* Trace returned 0 without a draw */
                    }
                }
            }
            const int wanted = __popcll(idle);
            poolPos += wanted < avail ? wanted : avail;
            idle = __ballot(!pathActive);
        }
