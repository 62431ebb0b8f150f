/* Stand-alone host test of ray-tracing_amd/csrc/rt_query_launch.h (the HIP-free half of include/rt_query.h): block and grid arithmetic,
 * the byte-size overflow guard, the overlap predicate and the argument checks.  tests/test_query.py builds it with
 * -fsanitize=address,undefined and runs it; it prints QUERY_LAUNCH_OK and exits 0, or names the first check that failed. */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ray-tracing_amd/csrc/rt_query_launch.h"

static int g_failed = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                        \
        }                                                                      \
    } while (0)

static void test_blocks_and_grid()
{
    using namespace rt_qr;
    CHECK(blocks(0) == 0);
    CHECK(blocks(1) == 1);
    CHECK(blocks(63) == 1);
    CHECK(blocks(64) == 1);
    CHECK(blocks(65) == 2);
    CHECK(blocks(RT_QUERY_MAX_RAYS) == (1ll << 20));
    CHECK(blocks(-5) == 0);
    /* the last lane index of the last block fits an int: the kernel's ray index is one */
    CHECK(blocks(RT_QUERY_MAX_RAYS) * RAYS_PER_BLOCK <= (long long)INT_MAX);
    const long long resident = 256 * 24;
    CHECK(grid(blocks(0), resident, 0) == 0);
    CHECK(grid(blocks(1), resident, 0) == 1);
    CHECK(grid(blocks(63), resident, 0) == 1);
    CHECK(grid(blocks(64), resident, 0) == 1);
    CHECK(grid(blocks(65), resident, 0) == 2);
    CHECK(grid(blocks(RT_QUERY_MAX_RAYS), resident, 0) == resident);
    /* RT_GRID in place of the resident waves, still capped at the blocks */
    CHECK(grid(blocks(64 * 5 + 3), resident, 2) == 2);
    CHECK(grid(blocks(65), resident, 100) == 2);
    CHECK(grid(blocks(0), resident, 2) == 0);
    CHECK(grid(blocks(1000), 0, 0) == 1); /* an occupancy query that answered 0 still launches */
    CHECK(grid(blocks(1000), resident, -3) == 16);
    /* every block is visited exactly once by a grid-stride walk */
    for (long long n : {1ll, 63ll, 64ll, 65ll, 130ll, 323ll}) {
        for (int over : {0, 1, 2, 7}) {
            const long long nb = blocks(n), g = grid(nb, 4, over);
            std::vector<int> seen((size_t)nb, 0);
            for (long long w = 0; w < g; w++)
                for (long long b = w; b < nb; b += g) seen[(size_t)b]++;
            for (long long b = 0; b < nb; b++) CHECK(seen[(size_t)b] == 1);
        }
    }
}

static void test_byte_size()
{
    using namespace rt_qr;
    size_t bytes = 1;
    CHECK(byte_size(0, 48, &bytes) && bytes == 0);
    CHECK(byte_size(1, 48, &bytes) && bytes == 48);
    CHECK(byte_size(RT_QUERY_MAX_RAYS, sizeof(RtRayHit), &bytes) && bytes == (size_t)48 << 26);
    CHECK(byte_size(RT_QUERY_MAX_RAYS, sizeof(RtRay), &bytes) && bytes == (size_t)32 << 26);
    CHECK(!byte_size(-1, 48, &bytes) && bytes == 0);
    CHECK(!byte_size(LLONG_MAX, 48, &bytes) && bytes == 0);
    CHECK(byte_size((long long)(SIZE_MAX / 48 > (size_t)LLONG_MAX ? (size_t)LLONG_MAX : SIZE_MAX / 48), 48, &bytes));
    if (SIZE_MAX / 48 < (size_t)LLONG_MAX) CHECK(!byte_size((long long)(SIZE_MAX / 48) + 1, 48, &bytes) && bytes == 0);
    CHECK(byte_size(LLONG_MAX, 0, &bytes) && bytes == 0);
    CHECK(byte_size(LLONG_MAX, 1, &bytes) == ((unsigned long long)LLONG_MAX <= (unsigned long long)SIZE_MAX));
}

static void test_overlap()
{
    using namespace rt_qr;
    static char buf[256];
    CHECK(!ranges_overlap(buf, 64, buf + 64, 64));      /* touching */
    CHECK(!ranges_overlap(buf + 64, 64, buf, 64));
    CHECK(ranges_overlap(buf, 65, buf + 64, 64));       /* one byte shared */
    CHECK(ranges_overlap(buf + 64, 64, buf, 65));
    CHECK(ranges_overlap(buf, 256, buf + 32, 16));      /* nested */
    CHECK(ranges_overlap(buf + 32, 16, buf, 256));
    CHECK(ranges_overlap(buf, 64, buf, 64));            /* identical */
    CHECK(!ranges_overlap(buf, 32, buf + 128, 32));     /* disjoint */
    CHECK(!ranges_overlap(buf + 128, 32, buf, 32));
    CHECK(!ranges_overlap(buf, 0, buf, 64));            /* empty */
    CHECK(!ranges_overlap(buf + 8, 64, buf + 16, 0));
    /* a range that ends at the top of the address space */
    const void* top = (const void*)(UINTPTR_MAX - 15);
    CHECK(!ranges_overlap(top, 16, buf, 256));
    CHECK(ranges_overlap(top, 16, (const void*)(UINTPTR_MAX - 3), 4));
    CHECK(!ranges_overlap((const void*)(UINTPTR_MAX - 31), 16, top, 16));
}

static void test_check_batch()
{
    using namespace rt_qr;
    static RtRay rays[4];
    static RtRayHit hits[4];
    static uint32_t occ[4];
    size_t rb = 0, ob = 0;
    const char* why = nullptr;
    CHECK(check_batch(rays, 4, hits, sizeof(RtRayHit), &rb, &ob, &why) == RT_OK && rb == 128 && ob == 192 && why[0] == 0);
    CHECK(check_batch(rays, 4, occ, sizeof(uint32_t), &rb, &ob, &why) == RT_OK && rb == 128 && ob == 16);
    CHECK(check_batch(nullptr, 0, nullptr, sizeof(RtRayHit), &rb, &ob, &why) == RT_OK && rb == 0 && ob == 0);
    CHECK(check_batch(rays, -1, hits, sizeof(RtRayHit), &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]);
    CHECK(check_batch(rays, RT_QUERY_MAX_RAYS + 1, hits, sizeof(RtRayHit), &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]);
    CHECK(check_batch(rays, INT_MAX, hits, sizeof(RtRayHit), &rb, &ob, &why) == RT_ERR_INVALID_ARG);
    CHECK(check_batch(nullptr, 1, hits, sizeof(RtRayHit), &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]);
    CHECK(check_batch(rays, 1, nullptr, sizeof(RtRayHit), &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]);
    CHECK(check_batch(rays, 2, (char*)rays + 32, sizeof(uint32_t), &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]); /* inside the rays */
    CHECK(check_batch(rays, 2, (char*)rays + 64, sizeof(uint32_t), &rb, &ob, &why) == RT_OK);                         /* right behind them */
    CHECK(check_batch(rays, 4, rays, sizeof(RtRayHit), &rb, &ob, &why) == RT_ERR_INVALID_ARG);                        /* in place */
}

int main()
{
    test_blocks_and_grid();
    test_byte_size();
    test_overlap();
    test_check_batch();
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    puts("QUERY_LAUNCH_OK");
    return 0;
}
