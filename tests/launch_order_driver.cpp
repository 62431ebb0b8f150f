// Host-only driver of ray-tracing_amd/csrc/rt_launch_order.h for tests/test_launch_order.py.
//
// A fake backend records what LaunchOrder issues into a happens-before model of the context's two streams (stream order, event
// edges, host synchronises) and the buffers each step touches; a small context mirrors launch_frames' buffer preparation around
// place() / run().  Commands:
//   run <ops> [options]          one sequence: per-op step lists, then VIOLATION / ORDERED lines
//   random <seed> <n> [options]  n seeded random sequences: the first violating one, or "clean n"
//   shortest <len> <alphabet> [options]  every sequence over the alphabet up to len ops, shortest first: the first violating one
// Ops (space separated): f = a single frame; F<n><k> = a launch of n frames, k = p pooled, g group, s single-wave (1 <= n <= 64): the
// workgroup shape comes from rt_launch_plan.h (launch_shape) for a 1080p FLAT scene with the chain pool / a BVH scene with a top-of-tree
// cache / a FLAT scene without the pool;
// w = non-render work (upload, reset, read-back); r = resize; c / o = switch to a caller's stream / back to the own stream.
// Options: two=0 (RT_TWO_STREAMS=0), lpt=0, alt=0 (RT_ALTERNATE=0), slab1=0 (the second staging slab does not fit),
// slabs=0 (no slab fits), drop=<event> (the backend drops that event's waits), steady=<k> (fused launches k, k+1, ... and their
// successors: the trace kernels of two consecutive ones on different streams must not be ordered).
#include "../ray-tracing_amd/csrc/rt_launch_order.h"
#include "../ray-tracing_amd/csrc/rt_launch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace rt_order;

static const char* kEventNames[EVENT_COUNT] = {"FORK", "JOIN", "SORT", "ORDER_RETIRE0", "ORDER_RETIRE1",
                                                "ACC_WRITER0", "ACC_WRITER1", "ACC_FULL0", "ACC_FULL1"};

// buffers: the order buffers, the sort's key snapshot, per stream the staging slab / pixel records / tile counter, the accumulation
// and frame buffers (ACC).  Tile-cost atomics are exempt (every kernel raises them, the sort reads a snapshot).
enum Res { ORDER0, ORDER1, KEY, STAGING0, STAGING1, PXREC0, PXREC1, COUNTER0, COUNTER1, ACC, RES_COUNT };
static const char* kResNames[RES_COUNT] = {"order0", "order1", "key", "staging0", "staging1", "pxrec0", "pxrec1", "counter0", "counter1", "acc"};

struct Access {
    int res;
    bool write;
    int half = -1;  // ACC: -1 = whole image, else the half of a two-part frame ...
    int epoch = 0;  // ... under the tile order of this sort epoch
};

struct Node {
    int stream, seq, op, launch;
    int vc[2];
    bool trace = false, staged = false;
    int part = -1;
    std::vector<Access> acc;
    std::string what;
};

static const int kTiles = 240 * 135;  // 1920 x 1080

static bool single_wave(char kind, int nFrames)
{
    rt_plan::SceneShape sc;
    sc.flat = kind != 'g';
    sc.stackEntries = sc.flat ? 0 : 20;
    sc.hotUnits = sc.flat ? 0u : 448u * 4u;
    sc.wavesPerGroup = RT_MAX_WAVES_PER_GROUP;
    sc.poolCells = kind == 'p' ? (int)RT_POOL_CELLS : 0;
    sc.poolWaves = RT_MAX_WAVES_PER_GROUP_FLAT;
    return rt_plan::launch_shape(sc, kTiles, nFrames).wavesPerGroup == 1;
}

struct Options {
    bool two = true, lpt = true, alt = true, slab1 = true, slabs = true;
    int steady = 0;  // > 0: also check that fused launches from this one on do not order the next one's trace kernel
    int drop = -1;
};

struct Sim final : Backend {
    Options opt;
    LaunchOrder order;
    std::vector<Node> nodes;
    int clock[2][2] = {{0, 0}, {0, 0}};  // what each stream has been ordered after: per stream, nodes [1, clock] of it
    int eventClock[EVENT_COUNT][2] = {};
    int issued[2] = {0, 0};
    int op = 0;
    std::string steps;                    // the record / wait / kernel list of the current op
    int epochOf[2] = {0, 0}, epochs = 0;  // order buffer -> sort epoch it holds
    int frames = 1, launches = 0;         // frames of the launch being issued, launches so far
    // the context's buffers, as launch_frames prepares them
    bool recordsFor[3] = {false, false, false};
    bool orderMade = false, stagingUnavailable = false, slab[2] = {false, false}, callerStream = false;

    explicit Sim(const Options& o) : opt(o)
    {
        order.lpt = opt.lpt;
        order.alternate = opt.alt;
        order.set_two_streams(opt.two);
    }

    Node& node(int s, const std::string& what)
    {
        issued[s]++;
        clock[s][s] = issued[s];
        Node n;
        n.stream = s;
        n.seq = issued[s];
        n.op = op;
        n.launch = launches;
        n.vc[0] = clock[s][0];
        n.vc[1] = clock[s][1];
        n.what = what;
        nodes.push_back(n);
        return nodes.back();
    }
    void note(const std::string& t) { steps += (steps.empty() ? "" : " ") + t; }

    // ---- Backend
    int record(Event e, int s) override
    {
        eventClock[e][0] = clock[s][0];
        eventClock[e][1] = clock[s][1];
        note(std::string("+") + kEventNames[e] + "@" + std::to_string(s));
        return RT_OK;
    }
    int wait(int s, Event e) override
    {
        note(std::string(s ? "side" : "main") + "<" + kEventNames[e]);
        if (e == opt.drop) return RT_OK;
        for (int k = 0; k < 2; k++)
            if (eventClock[e][k] > clock[s][k]) clock[s][k] = eventClock[e][k];
        return RT_OK;
    }
    int sort(int s, int target) override
    {
        Node& n = node(s, "sort" + std::to_string(target));
        n.acc.push_back({ORDER0 + target, true});
        n.acc.push_back({KEY, true});
        epochOf[target] = ++epochs;
        note("sort" + std::to_string(target) + "@" + std::to_string(s));
        return RT_OK;
    }
    int trace(int s, int part, int parts) override
    {
        Node& n = node(s, "trace" + std::string(parts == 2 ? (part ? "B" : "A") : ""));
        n.trace = true;
        n.staged = frames > 1;
        n.part = parts == 2 ? part : -1;
        if (order.orderValid) n.acc.push_back({ORDER0 + order.orderCur, false});
        const int epoch = order.orderValid ? epochOf[order.orderCur] : 0;
        n.acc.push_back({PXREC0 + s, true});
        n.acc.push_back({COUNTER0 + s, true});
        if (frames > 1) n.acc.push_back({STAGING0 + s, true});
        else n.acc.push_back({ACC, true, n.part, epoch});
        note("trace" + std::string(parts == 2 ? (part ? "B" : "A") : "") + "@" + std::to_string(s));
        return RT_OK;
    }
    int accumulate(int s) override
    {
        Node& n = node(s, "accumulate");
        n.acc.push_back({STAGING0 + s, false});
        n.acc.push_back({ACC, true});
        note("acc@" + std::to_string(s));
        return RT_OK;
    }

    // ---- the context around the module
    void sync()  // hipStreamSynchronize(joined(ctx))
    {
        order.join(*this);
        for (int s = 0; s < 2; s++)
            for (int k = 0; k < 2; k++) clock[s][k] = issued[k];
        note("sync");
    }
    void nonrender(const char* what)  // a memset, upload or read on joined(ctx): touches everything
    {
        order.join(*this);
        Node& n = node(0, what);
        for (int r = 0; r < RES_COUNT; r++) n.acc.push_back({r, true});
        note(what);
    }
    void launch(int nFrames, char kind)
    {
        const int k = kind == 'p' ? 1 : kind == 'g' ? 2 : 0;
        if (!recordsFor[k]) { sync(); recordsFor[k] = true; }  // prepare_records: pixel records grow for a new workgroup shape
        if (opt.lpt && !orderMade) {                             // prepare_tile_order: buffers for this image size
            sync();
            nonrender("zero-costs");
            order.forget_order();
            orderMade = true;
        }
        Shape shape;
        shape.frames = nFrames;
        shape.singleWave = single_wave(kind, nFrames);
        shape.tiles = kTiles;
        const Placement p = order.place(shape);
        if (p.staged) {  // prepare_staging
            if (!stagingUnavailable && !slab[p.lane]) {
                sync();
                for (int sl = 0; sl < (p.split && order.alternate ? 2 : 1); sl++) {
                    const int b = sl == 0 ? p.lane : 1 - p.lane;
                    if (slab[b]) continue;
                    slab[b] = opt.slabs && (b == 0 || opt.slab1);
                    if (!slab[b] && b != p.lane) order.alternate = false;
                }
            }
            if (stagingUnavailable || !slab[p.lane]) {
                if (p.lane == 1) {
                    order.alternate = false;
                    order.stagedNext = 0;
                    return launch(nFrames, kind);
                }
                stagingUnavailable = true;
                for (int f = 0; f < nFrames; f++) launch(1, kind == 'g' ? 'g' : 's');
                return;
            }
        }
        frames = nFrames;
        launches++;
        order.run(p, *this);
    }
    void resize()  // rt_resize: buffers of the old size go, the accumulation buffer is cleared
    {
        sync();
        nonrender("clear");
        order.alternate = opt.alt;
        orderMade = stagingUnavailable = slab[0] = slab[1] = false;
    }
    void set_stream(bool caller)
    {
        sync();
        callerStream = caller;
        order.set_two_streams(opt.two && !caller);
    }

    bool apply(const std::string& t)
    {
        if (t == "f") launch(1, 's');
        else if (t[0] == 'F' && t.size() >= 3) {
            const int n = atoi(t.c_str() + 1);
            const char kind = t.back();
            if (n < 1 || n > 64 || (kind != 'p' && kind != 'g' && kind != 's')) return false;
            launch(n, kind);
        } else if (t == "w") nonrender("work");
        else if (t == "r") resize();
        else if (t == "c") set_stream(true);
        else if (t == "o") set_stream(false);
        else return false;
        return true;
    }

    bool hb(const Node& a, const Node& b) const { return b.vc[a.stream] >= a.seq; }

    static bool conflict(const Access& x, const Access& y)
    {
        if (x.res != y.res || (!x.write && !y.write)) return false;
        if (x.res != ACC || x.half < 0 || y.half < 0) return true;
        return x.half == y.half || x.epoch != y.epoch;  // halves of one epoch are disjoint pixel sets
    }

    // (a) every conflicting pair ordered in issue order; (b) the overlap the two streams exist for
    int check(std::vector<std::string>& out) const
    {
        int bad = 0;
        for (size_t j = 0; j < nodes.size(); j++)
            for (size_t i = 0; i < j; i++) {
                const Node &a = nodes[i], &b = nodes[j];
                const Access* hit = nullptr;
                for (const Access& x : a.acc) {
                    for (const Access& y : b.acc)
                        if (conflict(x, y)) { hit = &x; break; }
                    if (hit) break;
                }
                if (hit && !hb(a, b) && bad++ < 8) {
                    out.push_back("VIOLATION " + std::string(kResNames[hit->res]) + ": op" + std::to_string(a.op) + " " + a.what + "@" +
                                  std::to_string(a.stream) + " / op" + std::to_string(b.op) + " " + b.what + "@" + std::to_string(b.stream));
                }
            }
        for (size_t j = 0; j < nodes.size(); j++) {
            const Node& b = nodes[j];
            if (!b.trace) continue;
            size_t i = j;
            while (i-- > 0 && !nodes[i].trace) {}
            if (i >= j) continue;
            const Node& a = nodes[i];  // the trace kernel issued before b
            const bool halves = b.part == 1 && a.part == 0 && a.launch == b.launch;
            const bool fused = opt.steady > 0 && a.launch >= opt.steady && a.staged && b.staged && a.launch + 1 == b.launch && a.stream != b.stream;
            if ((halves || fused) && hb(a, b)) {
                bad++;
                out.push_back("ORDERED op" + std::to_string(a.op) + " " + a.what + "@" + std::to_string(a.stream) + " -> op" +
                              std::to_string(b.op) + " " + b.what + "@" + std::to_string(b.stream));
            }
        }
        return bad;
    }
};

static std::vector<std::string> split(const std::string& s)
{
    std::vector<std::string> v;
    size_t i = 0;
    while (i < s.size()) {
        while (i < s.size() && s[i] == ' ') i++;
        size_t j = i;
        while (j < s.size() && s[j] != ' ') j++;
        if (j > i) v.push_back(s.substr(i, j - i));
        i = j;
    }
    return v;
}

static std::string join(const std::vector<std::string>& v)
{
    std::string s;
    for (const std::string& t : v) s += (s.empty() ? "" : " ") + t;
    return s;
}

// runs a sequence; returns the number of findings (lines in *report when given)
static int run(const std::vector<std::string>& ops, const Options& opt, std::vector<std::string>* report)
{
    Sim sim(opt);
    for (const std::string& t : ops) {
        sim.op++;
        sim.steps.clear();
        if (!sim.apply(t)) {
            fprintf(stderr, "bad op '%s'\n", t.c_str());
            exit(2);
        }
        if (report) report->push_back(t + ": " + sim.steps);
    }
    std::vector<std::string> out;
    const int bad = sim.check(out);
    if (report) report->insert(report->end(), out.begin(), out.end());
    return bad;
}

static std::vector<std::string> random_ops(std::mt19937& rng, Options& opt)
{
    auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
    opt.two = pick(6) != 0;
    opt.lpt = pick(8) != 0;
    opt.alt = pick(6) != 0;
    opt.slab1 = pick(6) != 0;
    opt.slabs = pick(10) != 0;
    std::vector<std::string> ops;
    const int n = 3 + pick(22);
    bool caller = false;
    for (int i = 0; i < n; i++) {
        const int r = pick(100);
        if (r < 30) ops.push_back("f");
        else if (r < 80) {
            const int frames = 2 + (pick(3) ? pick(15) : pick(63));
            ops.push_back("F" + std::to_string(frames > 64 ? 64 : frames) + "psgs"[pick(4)]);
        } else if (r < 90) ops.push_back("w");
        else if (r < 94) ops.push_back("r");
        else {
            ops.push_back(caller ? "o" : "c");
            caller = !caller;
        }
    }
    return ops;
}

static std::string options_text(const Options& o)
{
    std::string s;
    if (!o.two) s += " two=0";
    if (!o.lpt) s += " lpt=0";
    if (!o.alt) s += " alt=0";
    if (!o.slab1) s += " slab1=0";
    if (!o.slabs) s += " slabs=0";
    return s;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string cmd = argv[1];
    Options opt;
    int first = cmd == "run" ? 3 : 4;
    for (int i = first; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "two=0") opt.two = false;
        else if (a == "lpt=0") opt.lpt = false;
        else if (a == "alt=0") opt.alt = false;
        else if (a == "slab1=0") opt.slab1 = false;
        else if (a == "slabs=0") opt.slabs = false;
        else if (a.rfind("steady=", 0) == 0) opt.steady = atoi(a.c_str() + 7);
        else if (a.rfind("drop=", 0) == 0) {
            for (int e = 0; e < EVENT_COUNT; e++)
                if (a.substr(5) == kEventNames[e]) opt.drop = e;
            if (opt.drop < 0) return 2;
        } else return 2;
    }
    if (cmd == "run" && argc >= 3) {
        std::vector<std::string> report;
        run(split(argv[2]), opt, &report);
        for (const std::string& l : report) printf("%s\n", l.c_str());
        return 0;
    }
    if (cmd == "random" && argc >= 4) {
        std::mt19937 rng((unsigned)atoi(argv[2]));
        const int n = atoi(argv[3]);
        for (int i = 0; i < n; i++) {
            Options o = opt;
            const std::vector<std::string> ops = random_ops(rng, o);
            std::vector<std::string> report;
            if (run(ops, o, &report)) {
                printf("FOUND %s |%s\n", join(ops).c_str(), options_text(o).c_str());
                for (const std::string& l : report) printf("%s\n", l.c_str());
                return 0;
            }
        }
        printf("clean %d\n", n);
        return 0;
    }
    if (cmd == "shortest" && argc >= 4) {
        const int len = atoi(argv[2]);
        const std::vector<std::string> alphabet = split(argv[3]);
        const int k = (int)alphabet.size();
        for (int l = 1; l <= len; l++) {
            std::vector<int> idx(l, 0);
            for (;;) {
                std::vector<std::string> ops;
                for (int i : idx) ops.push_back(alphabet[i]);
                std::vector<std::string> report;
                if (run(ops, opt, &report)) {
                    printf("FOUND %s\n", join(ops).c_str());
                    for (const std::string& r : report) printf("%s\n", r.c_str());
                    return 0;
                }
                int p = l - 1;
                while (p >= 0 && ++idx[p] == k) idx[p--] = 0;
                if (p < 0) break;
            }
        }
        printf("clean\n");
        return 0;
    }
    return 2;
}
