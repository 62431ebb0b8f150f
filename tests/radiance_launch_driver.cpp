/* Stand-alone host test of ray-tracing_amd/csrc/rt_radiance_launch.h (the HIP-free half of include/rt_radiance.h): the argument checks,
 * the byte sizes with their overflow guard, the overlap predicate, blocks and grid, and the hand-out of blocks to the waves of a launch.
 * tests/test_radiance.py builds it with -fsanitize=address,undefined and runs it; it prints RADIANCE_LAUNCH_OK and exits 0, or names
 * the first check that failed. */
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ray-tracing_amd/csrc/rt_radiance_launch.h"

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
    using namespace rt_rd;
    CHECK(RAYS_PER_BLOCK == 64);
    CHECK(blocks(0) == 0);
    CHECK(blocks(1) == 1);
    CHECK(blocks(63) == 1);
    CHECK(blocks(64) == 1);
    CHECK(blocks(65) == 2);
    CHECK(blocks(RT_QUERY_MAX_RAYS) == (1ll << 20));
    CHECK(blocks(-5) == 0);
    const long long resident = 256 * 24;
    /* the kernel's ray index (an int) and its block index gridDim.x + ticket (an int): the largest of either fits */
    CHECK(blocks(RT_QUERY_MAX_RAYS) * RAYS_PER_BLOCK <= (long long)INT_MAX);
    CHECK(ticket_block(resident, (unsigned long long)(blocks(RT_QUERY_MAX_RAYS) + resident)) * RAYS_PER_BLOCK <= (long long)INT_MAX);
    CHECK(grid(blocks(0), resident, 0) == 0);
    CHECK(grid(blocks(1), resident, 0) == 1);
    CHECK(grid(blocks(63), resident, 0) == 1);
    CHECK(grid(blocks(64), resident, 0) == 1);
    CHECK(grid(blocks(65), resident, 0) == 2);
    CHECK(grid(blocks(RT_QUERY_MAX_RAYS), resident, 0) == resident);
    CHECK(grid(blocks(64 * 5 + 3), resident, 2) == 2); /* RT_GRID in place of the resident waves, still capped at the blocks */
    CHECK(grid(blocks(65), resident, 100) == 2);
    CHECK(grid(blocks(0), resident, 2) == 0);
    CHECK(grid(blocks(1000), 0, 0) == 1); /* an occupancy query that answered 0 still launches */
}

/* The hand-out as the kernel runs it: wave w starts on first_block(w); a wave that has used its block up draws a ticket from the shared
 * counter and stops at the first block >= nBlocks.  Whatever the order in which the waves draw — round robin, one wave drawing `greed`
 * tickets in a row, the last wave first — every block is handed out exactly once and every wave ends. */
static void test_hand_out()
{
    using namespace rt_rd;
    for (long long n : {1ll, 63ll, 64ll, 65ll, 130ll, 323ll, 4096ll + 7}) {
        for (int over : {0, 1, 2, 7}) {
            for (int greed : {1, 3}) {
                const long long nb = blocks(n), g = grid(nb, 4, over);
                CHECK(g >= 1 && g <= nb);
                std::vector<int> seen((size_t)nb, 0);
                std::vector<bool> ended((size_t)g, false);
                unsigned long long counter = 0;
                for (long long w = 0; w < g; w++) {
                    CHECK(first_block(w) < nb);
                    seen[(size_t)first_block(w)]++;
                }
                long long alive = g, turn = g - 1;
                while (alive > 0) {
                    if (!ended[(size_t)turn]) {
                        for (int k = 0; k < greed && !ended[(size_t)turn]; k++) {
                            const long long b = ticket_block(g, counter++);
                            if (b >= nb) { ended[(size_t)turn] = true; alive--; }
                            else seen[(size_t)b]++;
                        }
                    }
                    turn = (turn + g - 1) % g;
                }
                for (long long b = 0; b < nb; b++) CHECK(seen[(size_t)b] == 1);
                CHECK(counter == (unsigned long long)nb); /* nb - g blocks from tickets, and one losing ticket per wave */
                /* rays of the last block at or past n are never assigned: the kernel's test is index < n */
                CHECK((nb - 1) * RAYS_PER_BLOCK < n && nb * RAYS_PER_BLOCK >= n);
            }
        }
    }
}

static void test_byte_size_and_overlap()
{
    using namespace rt_qr; /* the shared helpers, at this pass's sizes */
    size_t bytes = 1;
    CHECK(byte_size(0, sizeof(RtRadiance), &bytes) && bytes == 0);
    CHECK(byte_size(1, sizeof(RtRadiance), &bytes) && bytes == 16);
    CHECK(byte_size(RT_QUERY_MAX_RAYS, sizeof(RtRadiance), &bytes) && bytes == (size_t)16 << 26);
    CHECK(byte_size(RT_QUERY_MAX_RAYS, sizeof(RtPathRay), &bytes) && bytes == (size_t)32 << 26);
    CHECK(!byte_size(-1, sizeof(RtRadiance), &bytes) && bytes == 0);
    CHECK(!byte_size(LLONG_MAX, sizeof(RtRadiance), &bytes) && bytes == 0);
    CHECK(!byte_size(LLONG_MAX, sizeof(RtPathRay), &bytes) && bytes == 0);
    if (SIZE_MAX / 16 < (size_t)LLONG_MAX) {
        CHECK(byte_size((long long)(SIZE_MAX / 16), 16, &bytes) && bytes == SIZE_MAX / 16 * 16);
        CHECK(!byte_size((long long)(SIZE_MAX / 16) + 1, 16, &bytes) && bytes == 0);
    }
    static char buf[256];
    CHECK(!ranges_overlap(buf, 64, buf + 64, 32));  /* records right behind the rays */
    CHECK(!ranges_overlap(buf + 32, 32, buf, 32));  /* records right in front of them */
    CHECK(ranges_overlap(buf, 64, buf + 48, 32));   /* the first record inside the last ray */
    CHECK(ranges_overlap(buf + 16, 32, buf, 64));   /* nested */
    CHECK(ranges_overlap(buf, 64, buf, 32));        /* in place */
    CHECK(!ranges_overlap(buf, 0, buf, 32));        /* empty */
    const void* top = (const void*)(UINTPTR_MAX - 15);
    CHECK(!ranges_overlap(top, 16, buf, 256));      /* a range that ends at the top of the address space */
    CHECK(ranges_overlap(top, 16, (const void*)(UINTPTR_MAX - 3), 4));
}

static void test_check_batch()
{
    using namespace rt_rd;
    static RtPathRay rays[4];
    static RtRadiance out[4];
    size_t rb = 7, ob = 7;
    const char* why = nullptr;
    CHECK(check_batch(rays, 4, out, &rb, &ob, &why) == RT_OK && rb == 128 && ob == 64 && why[0] == 0);
    CHECK(check_batch(rays, 1, out, &rb, &ob, &why) == RT_OK && rb == 32 && ob == 16);
    CHECK(check_batch(nullptr, 0, nullptr, &rb, &ob, &why) == RT_OK && rb == 0 && ob == 0);
    CHECK(check_batch(rays, 0, out, &rb, &ob, &why) == RT_OK && rb == 0 && ob == 0);
    CHECK(check_batch(rays, -1, out, &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]);
    CHECK(check_batch(rays, INT_MIN, out, &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]);
    CHECK(check_batch(rays, RT_QUERY_MAX_RAYS + 1, out, &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]);
    CHECK(check_batch(rays, INT_MAX, out, &rb, &ob, &why) == RT_ERR_INVALID_ARG);
    CHECK(check_batch(nullptr, 1, out, &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]);
    CHECK(check_batch(rays, 1, nullptr, &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]);
    CHECK(check_batch(rays, 2, (char*)rays + 32, &rb, &ob, &why) == RT_ERR_INVALID_ARG && why[0]); /* inside the rays */
    CHECK(check_batch(rays, 2, (char*)rays + 64, &rb, &ob, &why) == RT_OK);                         /* right behind them */
    CHECK(check_batch(rays + 1, 3, rays, &rb, &ob, &why) == RT_ERR_INVALID_ARG);                    /* 48 bytes of records reach into the rays */
    CHECK(check_batch(rays + 1, 2, rays, &rb, &ob, &why) == RT_OK);                                 /* 32 bytes end where they start */
    CHECK(check_batch(rays + 1, 1, rays, &rb, &ob, &why) == RT_OK);
    CHECK(check_batch(rays, 4, rays, &rb, &ob, &why) == RT_ERR_INVALID_ARG);                        /* in place */
    /* 2^26 rays pass the count and size checks (nothing is dereferenced); the ranges named here are disjoint */
    CHECK(check_batch((const void*)0x10000000, RT_QUERY_MAX_RAYS, (const void*)0x100000000000ull, &rb, &ob, &why) == RT_OK && rb == (size_t)32 << 26 &&
          ob == (size_t)16 << 26);
}

int main()
{
    test_blocks_and_grid();
    test_hand_out();
    test_byte_size_and_overlap();
    test_check_batch();
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    puts("RADIANCE_LAUNCH_OK");
    return 0;
}
