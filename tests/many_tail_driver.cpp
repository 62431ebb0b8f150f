/* Stand-alone host test of the order in which a lane of the > 64-model kernels visits its models (ray-tracing_amd/csrc/rt_kernels.h,
 * begin_intersect's candidate words and phase A of traverse), around rt_plan::next_unfiltered_model of rt_launch_plan.h — the one
 * expression the kernel's vote and its phase A share.  The lane below is the kernel's restated: a 63-bit register mask for models
 * 0 ... 62 with bit 63 for "the extension holds more", a summary word and up to 32 extension words for models 63 ... 1086, then the
 * models no filter sees, in index order.  For n models and a set of kept candidates it must visit exactly the kept candidates and every
 * unfiltered model, each once, in increasing order, and stop.  tests/test_many_models.py builds it plainly and with
 * -fsanitize=address,undefined and runs it; it prints MANY_TAIL_OK and exits 0, or names the first check that failed. */
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../ray-tracing_amd/csrc/rt_launch_plan.h"

static int g_failed = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            if (g_failed < 20) fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                        \
        }                                                                      \
    } while (0)

struct Lane {
    unsigned long long cand = 0;
    uint32_t ext[1 + RT_MAX_FILTER_EXT_WORDS] = {0}; /* extBase[w * RT_WAVE]: the summary, then the words */
    int m = -1;
};

/* begin_intersect, the > 64-model arm: what the chunk walk leaves for the kept models */
static Lane begin(const std::vector<char>& keep, const rt_plan::Filtering& f)
{
    Lane t;
    for (int w = 0; w <= f.extWords; w++) t.ext[w] = 0u;
    for (int m = 0; m < f.nFiltered; m++) {
        if (m < 63) {
            t.cand |= (keep[(size_t)m] ? 1ull : 0ull) << m;
        } else if (keep[(size_t)m]) {
            const int w = (m - 63) >> 5;
            CHECK(w < f.extWords);
            t.ext[1 + w] |= 1u << ((m - 63) & 31);
            t.ext[0] |= 1u << w;
            t.cand |= 1ull << 63;
        }
    }
    return t;
}

/* the vote's "done" test and phase A, until the lane is done; the models it visited */
static std::vector<int> walk(Lane t, int nModels, int nFiltered)
{
    std::vector<int> visited;
    for (int step = 0; step <= nModels; step++) {
        if (!t.cand && rt_plan::next_unfiltered_model(t.m, nFiltered) >= nModels) return visited;
        const unsigned long long regBits = t.cand & 0x7fffffffffffffffull;
        if (regBits) {
            t.m = __builtin_ffsll((long long)regBits) - 1;
            t.cand &= t.cand - 1;
        } else if (t.cand) {
            uint32_t summary = t.ext[0];
            const int w = __builtin_ffs((int)summary) - 1;
            CHECK(w >= 0 && w < RT_MAX_FILTER_EXT_WORDS);
            if (w < 0 || w >= RT_MAX_FILTER_EXT_WORDS) return visited;
            uint32_t word = t.ext[1 + w];
            t.m = 63 + 32 * w + (__builtin_ffs((int)word) - 1);
            word &= word - 1;
            t.ext[1 + w] = word;
            if (!word) {
                summary &= summary - 1;
                t.ext[0] = summary;
                if (!summary) t.cand = 0;
            }
        } else {
            t.m = rt_plan::next_unfiltered_model(t.m, nFiltered);
        }
        CHECK(t.m >= 0 && t.m < nModels); /* the kernel reads models[t.m] next */
        if (t.m < 0 || t.m >= nModels) return visited;
        visited.push_back(t.m);
    }
    const bool doneWithinNModelsSteps = false;
    CHECK(doneWithinNModelsSteps);
    return visited;
}

static void check_set(int n, const std::vector<char>& keep)
{
    const rt_plan::Filtering f = rt_plan::filtering(n);
    std::vector<int> want;
    for (int m = 0; m < n; m++)
        if (m >= f.nFiltered || keep[(size_t)m]) want.push_back(m);
    const std::vector<int> got = walk(begin(keep, f), n, f.nFiltered);
    CHECK(got == want);
    for (size_t i = 1; i < got.size(); i++) CHECK(got[i] > got[i - 1]);
}

int main()
{
    for (int n : {65, 1087, 1088, 1300}) {
        const rt_plan::Filtering f = rt_plan::filtering(n);
        CHECK(f.nFiltered == (n < 1087 ? n : 1087) && f.extWords == (f.nFiltered - 63 + 31) / 32);
        /* the rule by itself: from model m the next unfiltered model is the first index behind both m and the filtered range */
        for (int m = -1; m < n; m++) {
            const int next = rt_plan::next_unfiltered_model(m, f.nFiltered);
            CHECK(next == (m + 1 > f.nFiltered ? m + 1 : f.nFiltered));
        }
        std::vector<char> none((size_t)n, 0), all((size_t)n, 1);
        check_set(n, none);
        check_set(n, all);
        { /* every index 0 ... n - 1 exactly once with every candidate kept */
            const std::vector<int> got = walk(begin(all, f), n, f.nFiltered);
            CHECK((int)got.size() == n);
            for (int m = 0; m < (int)got.size(); m++) CHECK(got[(size_t)m] == m);
        }
        std::vector<char> only = none, but = all;
        if (1086 < n) only[1086] = 1, but[1086] = 0;
        check_set(n, only);
        check_set(n, but);
        /* the last filtered model alone and all but it; the first and the last bit of every extension word; the register mask alone */
        std::vector<char> last = none, butLast = all, firsts = none, lasts = none, reg = none;
        last[(size_t)f.nFiltered - 1] = 1, butLast[(size_t)f.nFiltered - 1] = 0;
        for (int m = 63; m < f.nFiltered; m++) {
            if (((m - 63) & 31) == 0) firsts[(size_t)m] = 1;
            if (((m - 63) & 31) == 31) lasts[(size_t)m] = 1;
        }
        for (int m = 0; m < 63; m++) reg[(size_t)m] = 1;
        for (const std::vector<char>* s : {&last, &butLast, &firsts, &lasts, &reg}) check_set(n, *s);
        /* each extension word alone */
        for (int w = 0; w < f.extWords; w++) {
            std::vector<char> one = none;
            for (int m = 63 + 32 * w; m < 63 + 32 * (w + 1) && m < f.nFiltered; m++) one[(size_t)m] = 1;
            check_set(n, one);
        }
        std::mt19937 rng((unsigned)n);
        for (int it = 0; it < 200; it++) {
            std::vector<char> some((size_t)n, 0);
            const unsigned density = rng() % 101u;
            for (int m = 0; m < n; m++) some[(size_t)m] = (rng() % 100u) < density;
            check_set(n, some);
        }
    }
    if (g_failed) {
        fprintf(stderr, "%d checks failed\n", g_failed);
        return 1;
    }
    puts("MANY_TAIL_OK");
    return 0;
}
