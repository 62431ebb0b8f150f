/* rt_mis_launch.h — the host arithmetic of include/rt_mis.h's call, without HIP, so that a host test reaches it
 * (tests/mis_map_driver.cpp): the device copy of the reverse map (rt_light_table.h, build_map) and its bytes.  The rays, the records,
 * their checks and the blocks of a launch are rt_radiance_launch.h's, the table and its pick rule rt_nee_launch.h's; both are used as
 * they are.  The kernel is rt_kernels.h's rt_radiance_mis_kernel; the entry point lives in rt_context.hip, with the context.
 *
 * The device copy, one allocation of its own (not inside rt_nee::table_bytes): nObjects records of four words
 *     { base, triOffset, triCount, 0 }
 * — base: a sphere's entry, or the index of the word of a model's first triangle in the words that follow; NO_ENTRY: the object has no
 * entry — then one word per triangle of every model with an entry: its entry, or NO_ENTRY.  A hit (object o, triangle k) finds its
 * entry by two dependent loads: record o, then word base + (k - triOffset) when k - triOffset < triCount (else NO_ENTRY: no index
 * leaves the allocation whatever the hit holds). */
#ifndef RT_MIS_LAUNCH_H
#define RT_MIS_LAUNCH_H

#include "../../include/rt_mis.h"
#include "rt_light_table.h"
#include "rt_nee_launch.h"

namespace rt_mis {

enum : uint32_t { NO_ENTRY = RT_MIS_NO_ENTRY, OBJECT_WORDS = 4 };

static_assert((uint32_t)rt_lt::LightMap::NO_ENTRY == (uint32_t)NO_ENTRY, "one value for 'no entry'");

struct MapBytes {
    size_t objects = 0, triangles = 0, total = 0; /* triangles: byte offset of the triangle words; total: bytes (never 0, a multiple of 16) */
};

inline MapBytes map_bytes(size_t nObjects, size_t nTriangleWords)
{
    MapBytes mb;
    mb.objects = 0;
    mb.triangles = nObjects * OBJECT_WORDS * sizeof(uint32_t);
    mb.total = mb.triangles + ((nTriangleWords * sizeof(uint32_t) + 15) & ~(size_t)15);
    if (mb.total == 0) mb.total = 16;
    return mb;
}

/* the device copy of `map` as words: map_bytes(...).total / 4 of them */
inline void pack_map(const rt_lt::LightMap& map, std::vector<uint32_t>& words)
{
    const MapBytes mb = map_bytes(map.objects.size(), map.triangles.size());
    words.assign(mb.total / sizeof(uint32_t), 0u);
    for (size_t o = 0; o < map.objects.size(); o++) {
        words[OBJECT_WORDS * o + 0] = map.objects[o];
        words[OBJECT_WORDS * o + 1] = map.triOffset[o];
        words[OBJECT_WORDS * o + 2] = map.triCount[o];
    }
    const size_t base = mb.triangles / sizeof(uint32_t);
    for (size_t k = 0; k < map.triangles.size(); k++) words[base + k] = map.triangles[k];
}

/* entry(object, triangle) on the packed words: the function body the kernel (rt_kernels.h, mis_entry) and the host test both run.
 * object in [0, nObjects); sphere: the object is a sphere (its record's base is the entry). */
#if defined(__HIPCC__)
__host__ __device__
#endif
inline uint32_t entry_of(const uint32_t* words, const uint32_t* triWords, const int object, const bool sphere, const int triangle)
{
    const uint32_t* const rec = words + (size_t)OBJECT_WORDS * (size_t)object;
    const uint32_t base = rec[0];
    if (sphere || base == (uint32_t)NO_ENTRY) return base;
    const uint32_t rel = (uint32_t)triangle - rec[1];
    if (!(rel < rec[2])) return (uint32_t)NO_ENTRY;
    return triWords[(size_t)base + rel];
}

} // namespace rt_mis

#endif /* RT_MIS_LAUNCH_H */
