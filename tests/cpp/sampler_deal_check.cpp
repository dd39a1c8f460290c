// Host check of the sampler's even dealing (spt::DealRule, spt_internal.h) and a 64-lane
// host model of coop_ball_vector (spt_path.h) against the sequential loop of
// Random.hpp:115-127 as oracle/spt_oracle.c restates it (spo_ball_vector).
//
// 1. The dealing rule, exhaustively for np = 1..64: every lane helps a rank below np, a
//    rank's lanes are contiguous, the counts are 64 / np or one more (the first 64 mod np
//    ranks) and sum to 64, trial offsets run 0..count-1 in lane order, deal_start /
//    deal_count name exactly those lanes, and the table's q and rem equal the plain
//    division (the kernel divides nowhere: the rule is a table entry).
// 2. The model: the kernel's rounds restated lane by lane (round 0 or its skip, the
//    packed lane | trials << 6 word, the segment of the acceptance ballot, the trial
//    count a pending lane adds), with spt_device.h's splitmix and uniform arithmetic.
//    For random (state, need mask) cases the vector and the advanced state of every
//    needing lane equal the sequential loop's, and the other lanes' states are untouched.
// Exit 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "spt_internal.h"

extern "C" void spo_ball_vector(uint64_t *state, float out[4]);

namespace {

constexpr uint64_t kGamma = 0x9E3779B97F4A7C15ull;

// spt_device.h next_u32 / uniform_bits
uint32_t next_u32(uint64_t &st)
{
    st += kGamma;
    uint64_t z = st;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 31);
}
float uniform(uint64_t &st, float a, float b)
{
    const float f = std::fmin((float)next_u32(st), 0x1.fffffep+31f);
    return std::fmaf(f, 0x1p-32f * (b - a), a);
}
float lensq(const float v[3])
{
    volatile float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
    volatile float s = xx + yy;
    return s + zz;
}
uint64_t ballot(const bool p[64])
{
    uint64_t m = 0;
    for (int l = 0; l < 64; ++l) m |= (uint64_t)p[l] << l;
    return m;
}
uint32_t rank_of(uint64_t mask, uint32_t lane) { return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull)); }

// coop_ball_vector for a whole wave: st[l] in and out, r[l] the vectors; returns rounds
int model(uint64_t st[64], const bool need[64], float r[64][3], bool skip0)
{
    uint64_t st0[64];
    uint32_t jacc[64];
    std::memcpy(st0, st, sizeof st0);
    const uint64_t needm = ballot(need);
    uint64_t pend;
    for (int l = 0; l < 64; ++l) r[l][0] = r[l][1] = r[l][2] = 0.f, jacc[l] = 0;
    if (skip0 && __builtin_popcountll(needm) <= 32) {
        pend = needm;
    } else {
        bool p[64];
        for (int l = 0; l < 64; ++l) {
            uint64_t t = st0[l];
            r[l][0] = uniform(t, -0.5f, 0.5f);
            r[l][1] = uniform(t, -0.5f, 0.5f);
            r[l][2] = uniform(t, -0.5f, 0.5f);
            p[l] = need[l] && lensq(r[l]) < 0.25f;
        }
        pend = ballot(p);
        for (int l = 0; l < 64; ++l) jacc[l] = (pend >> l & 1) ? 1u : 0u;
    }
    int rounds = 0;
    uint32_t lds[64] = {};
    while (pend != 0ull) {
        ++rounds;
        const spt::DealRule dr = spt::kDealTable.e[__builtin_popcountll(pend)];
        for (uint32_t l = 0; l < 64; ++l)
            if (pend >> l & 1) lds[rank_of(pend, l)] = (jacc[l] << 6) | l;
        float c[64][3];
        bool a[64];
        for (uint32_t l = 0; l < 64; ++l) {
            uint32_t pidx, tt;
            spt::deal_lane(dr, l, pidx, tt);
            const uint32_t w = lds[pidx];
            uint64_t b = st0[w & 63u] + (uint64_t)(3u * ((w >> 6) + tt)) * kGamma;
            c[l][0] = uniform(b, -0.5f, 0.5f);
            c[l][1] = uniform(b, -0.5f, 0.5f);
            c[l][2] = uniform(b, -0.5f, 0.5f);
            a[l] = !(lensq(c[l]) < 0.25f);
        }
        const uint64_t acc = ballot(a);
        bool still[64];
        for (uint32_t l = 0; l < 64; ++l) {
            const bool is_p = pend >> l & 1;
            still[l] = false;
            if (!is_p) continue;
            const uint32_t rank = rank_of(pend, l);
            const uint32_t start = spt::deal_start(dr, rank), cnt = spt::deal_count(dr, rank);
            const uint64_t seg = acc >> (start & 63u);
            const uint32_t tstar = seg != 0ull ? (uint32_t)__builtin_ctzll(seg) : 64u;
            const bool found = tstar < cnt;
            if (found) std::memcpy(r[l], c[start + tstar], sizeof r[l]);
            jacc[l] += found ? tstar : cnt;
            still[l] = !found;
        }
        pend = ballot(still);
    }
    for (int l = 0; l < 64; ++l)
        if (need[l]) st[l] = st0[l] + (uint64_t)(3u * (jacc[l] + 1u)) * kGamma;
    return rounds;
}

}  // namespace

int main()
{
    // ---- 1. the dealing rule
    for (uint32_t np = 1; np <= 64; ++np) {
        const spt::DealRule dr = spt::kDealTable.e[np];
        const uint32_t q = 64u / np, rem = 64u % np;
        if (dr.q != q || dr.rem != rem || dr.q * np + dr.rem != 64u) {
            std::printf("FAIL rule np=%u q=%u rem=%u\n", np, dr.q, dr.rem);
            return 1;
        }
        uint32_t count[64] = {}, prev_rank = 0, total = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            uint32_t rank, tt;
            spt::deal_lane(dr, lane, rank, tt);
            // contiguous and in rank order: the rank never decreases and steps by at most one
            if (rank >= np || rank < prev_rank || rank > prev_rank + 1u || (lane == 0 && rank != 0) ||
                tt != count[rank] || spt::deal_start(dr, rank) + tt != lane || tt >= spt::deal_count(dr, rank)) {
                std::printf("FAIL deal np=%u lane=%u -> rank %u offset %u\n", np, lane, rank, tt);
                return 1;
            }
            prev_rank = rank;
            ++count[rank];
        }
        for (uint32_t k = 0; k < np; ++k) {
            total += count[k];
            if (count[k] != q + (k < rem ? 1u : 0u) || count[k] != spt::deal_count(dr, k)) {
                std::printf("FAIL count np=%u rank=%u: %u\n", np, k, count[k]);
                return 1;
            }
        }
        if (total != 64u) {
            std::printf("FAIL total np=%u: %u\n", np, total);
            return 1;
        }
    }
    // ---- 2. the model against the sequential loop
    uint64_t z = 0x243F6A8885A308D3ull;
    auto rnd = [&]() { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return z; };
    long rounds = 0;
    for (int cse = 0; cse < 2000; ++cse) {
        uint64_t mask;
        switch (cse % 8) {
        case 0: mask = 1ull << (rnd() & 63); break;                        // 1 lane
        case 1: mask = ~0ull; break;                                       // 64 lanes
        case 2: mask = 0x5555555555555555ull << (rnd() & 1); break;        // 32 lanes
        case 3: mask = 0x5555555555555555ull | (1ull << (2 * (rnd() & 31) + 1)); break;  // 33 lanes
        case 4: mask = rnd() & rnd() & rnd(); break;                       // few
        case 5: mask = rnd() | rnd(); break;                               // many
        default: mask = rnd(); break;
        }
        const int want_bits[] = {1, 64, 32, 33};
        if (cse % 8 < 4 && __builtin_popcountll(mask) != want_bits[cse % 8]) {
            std::printf("FAIL case mask %d\n", cse);
            return 1;
        }
        uint64_t st[64], before[64];
        bool need[64];
        float r[64][3];
        for (int l = 0; l < 64; ++l) {
            st[l] = before[l] = rnd();
            need[l] = mask >> l & 1;
        }
        for (int skip0 = 0; skip0 < 2; ++skip0) {
            std::memcpy(st, before, sizeof st);
            rounds += model(st, need, r, skip0 != 0);
            for (int l = 0; l < 64; ++l) {
                if (!need[l]) {
                    if (st[l] != before[l]) {
                        std::printf("FAIL case %d lane %d: state of an idle lane changed\n", cse, l);
                        return 1;
                    }
                    continue;
                }
                uint64_t s = before[l];
                float want[4];
                spo_ball_vector(&s, want);
                if (s != st[l] || std::memcmp(want, r[l], 12) != 0) {
                    std::printf("FAIL case %d skip0=%d lane %d: state %016llx want %016llx, vector (%a %a %a) want (%a %a %a)\n",
                                cse, skip0, l, (unsigned long long)st[l], (unsigned long long)s, r[l][0], r[l][1], r[l][2],
                                want[0], want[1], want[2]);
                    return 1;
                }
            }
        }
    }
    if (rounds == 0) {
        std::printf("FAIL no cooperative round ran\n");
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
