// Host driver of ray-tracing_amd/csrc/rt_adaptive_math.h and of the HIP-free half of rt_adaptive_launch.h for tests/test_adaptive.py:
// the per-pixel error with the very function the selection kernel calls, then a serial tile maximum and a serial list; the check of a
// caller's tile list; the check of the parameters.
//
// Input (binary, little endian):  int32 mode, then
//   mode 0 (select):  int32 W, H;  float32 threshold, darkFloor;  int32 minFrames, maxFrames;  W*H x 4 float32 twice: the sum, the moments
//   mode 1 (list):    int32 W, rows, n;  n x uint32
//   mode 2 (params):  32 bytes: an RtAdaptiveParams
// Output (binary, to stdout):
//   mode 0:  uint32 tiles_active, pixels_active;  W*H float32 (the pixels' errors);  tiles_total float32 (the tiles' errors);
//            tiles_active uint32 (the list)
//   mode 1:  int64 (0, or 1 + the index of the first bad entry);  uint32 pixels
//   mode 2:  int32 status
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../ray-tracing_amd/csrc/rt_adaptive_launch.h"

static bool get(void* p, size_t size, size_t count) { return fread(p, size, count, stdin) == count; }
static bool put(const void* p, size_t size, size_t count) { return fwrite(p, size, count, stdout) == count; }

static int select_mode()
{
    int32_t dim[2], frames[2];
    float par[2];
    if (!get(dim, 4, 2) || !get(par, 4, 2) || !get(frames, 4, 2)) return 3;
    const int W = dim[0], H = dim[1];
    if (W < 1 || H < 1) return 4;
    const size_t n = (size_t)W * H;
    std::vector<rt_dn4> S(n), M(n);
    if (!get(S.data(), 16, n) || !get(M.data(), 16, n)) return 5;
    const int tilesX = rt_ad::tiles_x(W), tilesY = rt_ad::tiles_y(H);
    std::vector<float> err(n), tileErr((size_t)tilesX * tilesY, 0.0f);
    std::vector<uint32_t> list;
    uint32_t counts[2] = {0, 0};
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            err[i] = rt_ad_error(S[i], M[i], par[1], frames[0], frames[1]);
            float& t = tileErr[(size_t)(y / 8) * tilesX + x / 8];
            t = rt_ad_max(t, err[i]);
        }
    for (int ty = 0; ty < tilesY; ty++)
        for (int tx = 0; tx < tilesX; tx++)
            if (rt_ad_active(tileErr[(size_t)ty * tilesX + tx], par[0])) {
                list.push_back((uint32_t)(ty * tilesX + tx));
                counts[1] += rt_ad_tile_pixels(tx, ty, W, H);
            }
    counts[0] = (uint32_t)list.size();
    return put(counts, 4, 2) && put(err.data(), 4, n) && put(tileErr.data(), 4, tileErr.size()) && put(list.data(), 4, list.size()) ? 0 : 6;
}

static int list_mode()
{
    int32_t head[3];
    if (!get(head, 4, 3) || head[2] < 0) return 3;
    std::vector<uint32_t> tiles((size_t)head[2]);
    if (!get(tiles.data(), 4, tiles.size())) return 5;
    uint32_t pixels = 0;
    const int64_t bad = rt_ad::check_tiles(tiles.data(), head[2], head[0], head[1], &pixels);
    return put(&bad, 8, 1) && put(&pixels, 4, 1) ? 0 : 6;
}

static int params_mode()
{
    RtAdaptiveParams p;
    if (!get(&p, sizeof(p), 1)) return 3;
    rt_ad_job job;
    const char* why = "";
    const int32_t rc = rt_ad::check_params(&p, &job, &why);
    if (rc != 0 && !why[0]) return 7; /* every refusal says why */
    return put(&rc, 4, 1) ? 0 : 6;
}

int main()
{
    int32_t mode;
    if (!get(&mode, 4, 1)) return 3;
    return mode == 0 ? select_mode() : mode == 1 ? list_mode() : mode == 2 ? params_mode() : 4;
}
