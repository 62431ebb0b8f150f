/*
 * rt_records.h — the records of the HBM-resident scene (internal; plain C++, no HIP: the host-side scene preparation and its
 * host-compiled tests read them too).  What each record is for is told in the head of rt_device.h, which adds the kernels'
 * argument block to them.
 */
#ifndef RT_RECORDS_H
#define RT_RECORDS_H

#include <stdint.h>

#include "rt_launch_plan.h" /* RT_WAVE, RT_PIXEL_FIELDS, the workgroup maxima, the chain pool's sizes, RT_MIN_WAVES_PER_SIMD* */

#define RT_STACK_DEPTH 34            /* >= RT_MAX_BVH_DEPTH + 2 */
#define RT_COUNTER_SLOTS 1024        /* counters are spread over slots to avoid same-address atomics */
#define RT_N_PHASES 12
/* bytes of a wave's record in KArgs::pxCold: two float4 per lane (+ the traversal stack in the RT_GLOBAL_STACK experiment) */
#define RT_COLD_STRIDE_BYTES (2 * RT_WAVE * 16)
#define RT_COUNTER_FIELDS (8 + 2 * RT_N_PHASES + 4) /* ... + hot-cache steps, node-uniform steps (>= 48 lanes, >= 3/4 of the active lanes) */

/* Every record of the traversal is named by the 16-byte UNIT it starts at (rt_layout.h decides where the records lie):
 * node codes: bit31 = leaf.  leaf: [30:24] = triangle count (1..127), [23:0] = first unit of the leaf's run of DTri records
 * (three units each) relative to the model's triBase; count field 0 = indirect, [23:0] indexes bigLeaves {unit, count}.
 * inner: [30:0] = unit of the DPair in the pair space. */
#define RT_CODE_LEAF 0x80000000u
#define RT_CODE_NEXT_MODEL 0x7fffffffu /* traversal state: this model is finished */
#define RT_CODE_DONE 0x7ffffffeu       /* traversal state: every model visited (inner codes are below this) */
#define RT_CODE_MAX_INLINE_COUNT 127
#define RT_CODE_MAX_INLINE_START 0x00ffffffu

struct DPair {
    float aMin[3], aMax[3];
    float bMin[3], bMax[3];
    uint32_t codeA, codeB;
    uint32_t pad[2];
};
#define RT_PAIR_FORMAT 0
struct DTri {
    float ax, ay, az, abx;
    float aby, abz, acx, acy;
    float acz, fx, fy, fz;
};
struct DTriN {
    float n[9];
};
/* the kernels address these records with shifted 32-bit byte offsets (rt_kernels.h: unit << 4) */
static_assert(sizeof(DPair) == RT_PAIR_BYTES && sizeof(DTri) == 48 && sizeof(DTriN) == 36, "rt_kernels.h hard-codes the record sizes");
struct DModel {
    float w2l[12]; /* row r: m[r], m[4+r], m[8+r], m[12+r] of worldToLocal */
    float l2w[12];
    uint32_t rootCode;    /* 16-B aligned tail: (rootCode, triBase, cullBackface, -) */
    int32_t triBase;      /* first unit of the model's triangles in the triangle space */
    int32_t cullBackface; /* material.flag != GLASS (RC:355) */
    int32_t pad[5];
};
/* Conservative world-space stand-in for a model's root step (see begin_intersect): the union of
 * the root's two child boxes, transformed to world space and inflated; `always` = no filtering
 * (leaf root, or a matrix that cannot be inverted robustly). 32 B, scalar-loaded. */
struct DFilter {
    float bMin[3], bMax[3];
    uint32_t always;
    uint32_t innerRoot;
};
/* Two-level model hierarchy for scenes with more than 64 models (the "TLAS" of SURVEY.md §8(f)): models
 * are clustered in space (Morton order of their filter boxes) into chunks of up to 16; a chunk carries the
 * union of its members' filter boxes.  The lockstep filter first tests the chunk box and skips all 16 members
 * when no lane of the wave hits it.  Members are visited later in MODEL-INDEX order (bit masks), so the
 * clustering never changes results.  96 B, scalar-loaded. */
#define RT_CHUNK_MODELS 16
struct DChunk {
    float bMin[3], bMax[3];
    uint32_t always;      /* a member cannot be filtered: the chunk box is meaningless */
    uint32_t count;
    uint32_t innerRoots;  /* members whose root is an inner node (exact counters of skipped chunks) */
    uint32_t pad[3];
    uint32_t members[RT_CHUNK_MODELS];
};
struct DMaterial {
    float diffuseCol[4], emissionCol[4], specularCol[4], absorption[4];
    float absorptionStrength, emissionStrength, smoothness, specularProbability;
    float ior;
    int32_t flag;
    int32_t pad[2];
};

#endif
