// wedge_host_check.hip -- the host side of csrc/ss_wedge.hip under the host sanitizers, without a device: the tier rule, the table
// size and the slot hash of ss_wedge.hpp over their whole domain, and every argument check of the three entry points (each call
// below is rejected, or has nothing to do, before any launch).  Build and run from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I include -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all
//         tools/wedge_host_check.hip -o /tmp/wedge_host_check && /tmp/wedge_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../subgraph-sketching_amd/csrc/ss_wedge.hip"

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

int main()
{
    using namespace ss;
    // every source is served by exactly one tier, and a folded table is a power of two in [2 W, slots], never more than half full
    for (int slots = 1; slots <= kWedgeMaxSlots; slots <<= 1)
        for (int64_t W = 0; W <= 2 * kWedgeMaxSlots + 1; ++W) {
            CHECK(wedge_folds(W, slots) + wedge_emits(W, slots) == (W > 0));
            if (!wedge_folds(W, slots)) continue;
            const int m = wedge_table_slots(W, slots);
            CHECK(is_pow2(m) && m >= 2 && m <= slots && 2 * W <= m && (m == 2 || m < 4 * W));
            CHECK((1 << wedge_log2(m)) == m);
        }
    for (const int64_t W : {(int64_t)1 << 31, ((int64_t)1 << 62) - 1})  // (W(u) < 2^62: fewer than 2^31 edges of degree below 2^31)
        CHECK(!wedge_folds(W, kWedgeMaxSlots) && wedge_emits(W, 1) && wedge_emits(W, kWedgeMaxSlots));
    // the first slot lies inside the table for every table size, at both ends of the id range and in between
    for (int k = 1; (1 << k) <= kWedgeMaxSlots; ++k) {
        std::vector<int> hits((size_t)1 << k, 0);
        for (int64_t v = 0; v < ((int64_t)1 << 31); v += 65537) {
            const int h = wedge_slot((int32_t)v, k);
            CHECK(h >= 0 && h < (1 << k));
            ++hits[(size_t)h];
        }
        CHECK(wedge_slot(INT32_MAX, k) < (1 << k) && wedge_slot(0, k) == 0);
        int used = 0;
        for (const int n : hits) used += n > 0;
        CHECK(used > (1 << k) / 2);  // (32 768 probes: the multiply spreads them)
    }
    // known answers of the slot hash: the literal table KNOWN_SLOTS of tests/wedge_planted.py, whose Python twin finds the ids that the
    // planted collision graphs are made of -- change the hash and both fail
    // (tests/test_wedge_planted_host.py reads this table out of this file: keep `known[] = {`, the {v, k, slot} triples and the loop below)
    static const struct { int32_t v; int k, slot; } known[] = {
        {0, 1, 0}, {1, 1, 1}, {2, 1, 0}, {3, 1, 1}, {69999, 1, 1}, {2147483646, 1, 0}, {2147483647, 1, 1},
        {1, 6, 39}, {2, 6, 15}, {3, 6, 54}, {255, 6, 38}, {65536, 6, 30}, {123456789, 6, 31}, {2147483647, 6, 56},
        {1, 8, 158}, {5, 8, 23}, {256, 8, 55}, {4095, 8, 217}, {69999, 8, 194}, {1073741823, 8, 161}, {2147483647, 8, 225},
        {1, 12, 2531}, {2, 12, 966}, {3, 12, 3498}, {4096, 12, 1913}, {65535, 12, 3511}, {1000003, 12, 3444},
        {1073741824, 12, 1024}, {2147483646, 12, 1081}, {2147483647, 12, 3612}};
    for (const auto &a : known) CHECK(wedge_slot(a.v, a.k) == a.slot);
    // the entry points: all rejected (-1), or nothing to do (0), before any launch
    std::vector<int64_t> some(8, 0);
    std::vector<int32_t> col(8, 0);
    int64_t *p = some.data();
    int32_t *c = col.data();
    CHECK(ss_wedge_walks(p, c, (int64_t)1 << 31, p, 4, p, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_walks(p, c, -1, p, 4, p, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_walks(p, c, 8, p, -1, p, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_walks(p, c, 8, p, (int64_t)1 << 31, p, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_walks(nullptr, c, 8, p, 4, p, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_walks(p, nullptr, 8, p, 4, p, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_walks(p, c, 8, nullptr, 4, p, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_walks(p, c, 8, p, 4, nullptr, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_walks(p, c, 0, p, 4, p, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_walks(nullptr, nullptr, 8, nullptr, 0, nullptr, nullptr, nullptr) == SS_OK);
    for (const int32_t slots : {0, -64, 3, 48, 2 * SS_WEDGE_MAX_SLOTS, INT32_MAX, INT32_MIN}) {
        CHECK(ss_wedge_fold(p, c, 8, p, 4, p, p, slots, p, c, nullptr) == SS_ERR_INVALID_ARG);
        CHECK(ss_wedge_emit(p, c, 8, p, 4, p, p, slots, 1, p, nullptr) == SS_ERR_INVALID_ARG);
    }
    CHECK(ss_wedge_fold(p, c, 8, p, 4, nullptr, p, 64, p, c, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_fold(p, c, 8, p, 4, p, nullptr, 64, p, c, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_fold(p, c, 8, p, 4, p, p, 64, nullptr, c, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_fold(p, c, 8, p, 4, p, p, 64, p, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_fold(p, c, 8, p, 4, p, p, 1, p, c, nullptr) == SS_OK);  // (one slot: no source folds, no launch)
    CHECK(ss_wedge_fold(nullptr, nullptr, 8, nullptr, 0, nullptr, nullptr, 64, nullptr, nullptr, nullptr) == SS_OK);
    CHECK(ss_wedge_emit(p, c, 8, p, 4, nullptr, p, 64, 1, p, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_emit(p, c, 8, p, 4, p, nullptr, 64, 1, p, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_emit(p, c, 8, p, 4, p, p, 64, 1, nullptr, nullptr) == SS_ERR_INVALID_ARG);
    for (const int32_t slices : {0, -1, kWedgeMaxSlices + 1, INT32_MAX})
        CHECK(ss_wedge_emit(p, c, 8, p, 4, p, p, 64, slices, p, nullptr) == SS_ERR_INVALID_ARG);
    CHECK(ss_wedge_emit(nullptr, nullptr, 8, nullptr, 0, nullptr, nullptr, 64, 1, nullptr, nullptr) == SS_OK);
    std::puts("wedge_host_check ok");
    return 0;
}
