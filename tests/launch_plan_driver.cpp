// Host-only driver of ray-tracing_amd/csrc/rt_launch_plan.h for tests/test_launch_plan.py.
//
// Reads one request per line from stdin and answers each with one line of key=value pairs:
//   filter models=                                        -> nf ext
//   groups height= models= want= [hotkb=]                 -> wpg records
//   shape flat= stats= stack= ext= chunks= hot= wpg= pool= poolwaves= minitems= cus= tiles= frames=
//                                                         -> pooled many hot hotunits wpg threads poolcells wavedwords lds variant
//   many chunks= flat=                                    -> many
//   part tiles= frames= flat= spp= fg= grid= resident= wpg= part= parts= next=
//                                                         -> every PartPlan field
//   records resident= wpg= grid=                          -> waves
//   slab npix= budget= frames=                            -> frames
//   fuse ms= frames= npix= slab0= slab1=                  -> cap perframe
//   pin v=                                                -> cap
//   tuner flat= staged= frames= stats= since= ms0= ms1= n0= n1=  -> samples decision
//   queue seed= n=                                        -> "clean <launches>" or the first broken launch
// Absent keys are 0.
#include "../ray-tracing_amd/csrc/rt_launch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <vector>

using namespace rt_plan;

struct Req {
    std::map<std::string, std::string> kv;
    bool has(const char* k) const { return kv.count(k) != 0; }
    long long i(const char* k) const { return has(k) ? atoll(kv.at(k).c_str()) : 0; }
    double d(const char* k) const { return has(k) ? atof(kv.at(k).c_str()) : 0.0; }
};

static std::string part_line(const PartPlan& p)
{
    std::ostringstream o;
    o << "tiles=" << p.partTiles << " group=" << p.frameGroup << " shift=" << p.frameGroupShift << " groups=" << p.frameGroups << " items=" << p.items
      << " grid=" << p.grid << " gridwaves=" << p.gridWaves << " byindex=" << p.byIndex << " qstart=" << p.queueStart << " base=" << p.tileQueueBase
      << " next=" << p.queueNext;
    return o.str();
}

// One launch on the kernel's side (rt_kernels.h, rt_trace_kernel: the persistent loop's first position — `tile = gw` when
// gw < launchItems and !queueStart — and its queue fetch — `atomicAdd(c.tileQueue, 1) - c.tileQueueBase`, the wave stops fetching at the
// first position >= launchItems).  The waves fetch in a random interleaving.  Returns "" or what broke.
static std::string run_kernel(const PartPlan& p, unsigned long long& counter, std::mt19937& rng)
{
    std::vector<unsigned char> taken((size_t)p.items, 0);
    std::string bad;
    auto take = [&](long long pos) {
        if (pos < 0 || pos >= p.items) bad = "position " + std::to_string(pos) + " outside [0, " + std::to_string(p.items) + ")";
        else if (taken[(size_t)pos]++) bad = "position " + std::to_string(pos) + " taken twice";
    };
    for (unsigned long long gw = 0; gw < p.gridWaves && bad.empty(); gw++)
        if ((long long)gw < p.items && !p.queueStart) take((long long)gw);
    std::vector<unsigned long long> live(p.gridWaves);
    for (unsigned long long k = 0; k < p.gridWaves; k++) live[k] = k;
    while (!live.empty() && bad.empty()) {
        const size_t k = rng() % live.size();
        const long long pos = (long long)(counter++ - p.tileQueueBase);
        if (pos >= p.items) {  // this wave's overshoot: it fetches no more
            live[k] = live.back();
            live.pop_back();
        } else take(pos);
    }
    for (long long q = 0; q < p.items && bad.empty(); q++)
        if (!taken[(size_t)q]) bad = "position " + std::to_string(q) + " never taken";
    return bad;
}

// Seeded random launches on the context's two tile counters: every position of every launch taken once, the counter where the plan says
// the next launch starts, the parts' tiles disjoint and covering, the frame groups covering the frames, the grid within the pixel records.
static std::string queue(unsigned seed, int n)
{
    std::mt19937 rng(seed);
    auto pick = [&](long long lo, long long hi) { return lo + (long long)(rng() % (unsigned long long)(hi - lo + 1)); };
    unsigned long long counter[2] = {0, 0}, next[2] = {0, 0};
    int launches = 0;
    for (int i = 0; i < n; i++) {
        Work w;
        w.tiles = (int)(pick(0, 3) ? pick(1, 40000) : pick(1, 64));
        w.nFrames = (int)(pick(0, 2) ? 1 : pick(1, 64));
        w.flat = pick(0, 3) != 0;
        w.spp = pick(0, 9) ? (int)pick(1, 64) : 65536;
        w.wavesPerGroup = (int)std::vector<int>{1, 12, 16}[pick(0, 2)];
        w.residentGroups = pick(1, 2048);
        w.frameGroupOverride = pick(0, 4) ? 0 : (int)pick(1, 8);
        const int parts = w.tiles >= 2 ? (int)pick(1, 2) : 1;  // (rt_launch_order.h, place: two parts only for >= 2 tiles)
        std::vector<int> hit((size_t)w.tiles, 0);
        for (int part = 0; part < parts; part++) {
            const long long items = (long long)((w.tiles - part + parts - 1) / parts) * w.nFrames;
            const int g = (int)pick(0, 3);
            w.gridOverride = g == 0 ? 0 : g == 1 ? (int)pick(1, items) : (int)pick(items, items + 5000);
            const PartPlan p = plan_part(w, part, parts, next[part]);
            std::string bad;
            if (counter[part] != next[part]) bad = "counter " + std::to_string(counter[part]) + " != planned start " + std::to_string(next[part]);
            if (bad.empty()) bad = run_kernel(p, counter[part], rng);
            if (bad.empty() && counter[part] != p.queueNext)
                bad = "counter ends at " + std::to_string(counter[part]) + ", the plan says " + std::to_string(p.queueNext);
            if (bad.empty() && !(p.frameGroups * p.frameGroup >= w.nFrames && w.nFrames > (p.frameGroups - 1) * p.frameGroup))
                bad = "frame groups do not cover the frames";
            if (bad.empty() && p.gridWaves > (unsigned long long)record_waves(w.residentGroups, w.wavesPerGroup, w.gridOverride))
                bad = "more waves than pixel records";
            for (int q = 0; q < p.partTiles && bad.empty(); q++) {
                const long long e = (long long)q * parts + part;  // tile-order entry of queue position q (KArgs::orderStride / orderOffset)
                if (e >= w.tiles) bad = "tile entry " + std::to_string(e) + " beyond the image";
                else hit[(size_t)e]++;
            }
            if (!bad.empty()) {
                std::ostringstream o;
                o << "BROKEN launch " << i << " part " << part << "/" << parts << ": " << bad << " | tiles=" << w.tiles << " frames=" << w.nFrames
                  << " flat=" << w.flat << " spp=" << w.spp << " wpg=" << w.wavesPerGroup << " resident=" << w.residentGroups
                  << " fg=" << w.frameGroupOverride << " grid=" << w.gridOverride << " | " << part_line(p);
                return o.str();
            }
            next[part] = p.queueNext;
            launches++;
        }
        for (int t = 0; t < w.tiles; t++)
            if (hit[(size_t)t] != 1) return "BROKEN launch " + std::to_string(i) + ": tile entry " + std::to_string(t) + " in " + std::to_string(hit[(size_t)t]) + " parts";
    }
    return "clean " + std::to_string(launches);
}

static std::string answer(const std::string& cmd, const Req& r)
{
    std::ostringstream o;
    if (cmd == "filter") {
        const Filtering f = filtering((int)r.i("models"));
        o << "nf=" << f.nFiltered << " ext=" << f.extWords;
    } else if (cmd == "groups") {
        const GroupPlan g = plan_groups((int)r.i("height"), (int)r.i("models"), (int)r.i("want"), r.has("hotkb"), r.i("hotkb"));
        o << "wpg=" << g.wavesPerGroup << " records=" << g.cacheRecords;
    } else if (cmd == "shape") {
        SceneShape s;
        s.flat = r.i("flat");
        s.stats = r.i("stats");
        s.stackEntries = (int)r.i("stack");
        s.extWords = (int)r.i("ext");
        s.nChunks = (int)r.i("chunks");
        s.hotUnits = (uint32_t)r.i("hot");
        s.wavesPerGroup = (int)r.i("wpg");
        s.poolCells = (int)r.i("pool");
        s.poolWaves = (int)r.i("poolwaves");
        s.poolMinItems = (int)r.i("minitems");
        s.numCUs = (int)r.i("cus");
        const LaunchShape l = launch_shape(s, r.i("tiles"), (int)r.i("frames"));
        o << "pooled=" << l.pooled << " many=" << l.many << " hot=" << l.hot << " hotunits=" << l.hotUnits << " wpg=" << l.wavesPerGroup
          << " threads=" << l.blockThreads << " poolcells=" << l.poolCells << " wavedwords=" << l.waveLdsDwords << " lds=" << l.ldsBytes
          << " variant=" << l.variant;
    } else if (cmd == "many") {
        o << "many=" << many_models((int)r.i("chunks"), r.i("flat"));
    } else if (cmd == "part") {
        Work w;
        w.tiles = (int)r.i("tiles");
        w.nFrames = (int)r.i("frames");
        w.flat = r.i("flat");
        w.spp = (int)r.i("spp");
        w.frameGroupOverride = (int)r.i("fg");
        w.gridOverride = (int)r.i("grid");
        w.residentGroups = r.i("resident");
        w.wavesPerGroup = (int)r.i("wpg");
        o << part_line(plan_part(w, (int)r.i("part"), (int)r.i("parts"), (unsigned long long)r.i("next")));
    } else if (cmd == "records") {
        o << "waves=" << record_waves(r.i("resident"), (int)r.i("wpg"), (int)r.i("grid"));
    } else if (cmd == "slab") {
        o << "frames=" << slab_frames((size_t)r.i("npix"), (size_t)r.i("budget"), (int)r.i("frames"));
    } else if (cmd == "fuse") {
        const size_t slabs[2] = {(size_t)r.i("slab0"), (size_t)r.i("slab1")};
        const FuseCap f = fuse_cap((float)r.d("ms"), (int)r.i("frames"), (size_t)r.i("npix"), slabs);
        o << "cap=" << f.cap << " perframe=" << f.msPerFrame;
    } else if (cmd == "pin") {
        o << "cap=" << pinned_fuse_cap((int)r.i("v"));
    } else if (cmd == "tuner") {
        const double ms[2] = {r.d("ms0"), r.d("ms1")};
        const int n[2] = {(int)r.i("n0"), (int)r.i("n1")};
        o << "samples=" << tuner_samples(r.i("flat"), r.i("staged"), (int)r.i("frames"), r.i("stats"), r.i("since"))
          << " decision=" << tuner_decision(ms, n);
    } else if (cmd == "queue") {
        o << queue((unsigned)r.i("seed"), (int)r.i("n"));
    } else {
        o << "ERROR unknown request " << cmd;
    }
    return o.str();
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, tok;
        in >> cmd;
        Req r;
        while (in >> tok) {
            const size_t eq = tok.find('=');
            if (eq != std::string::npos) r.kv[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        printf("%s\n", answer(cmd, r).c_str());
    }
    return 0;
}
