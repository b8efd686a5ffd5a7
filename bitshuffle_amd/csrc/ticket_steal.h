// ticket_steal.h -- the arithmetic of block-ticket stealing (struct Tickets,
// bshuf_dev.h): how many tickets a shard's counter may hand out, and which
// shard a wave whose own has run out draws from.  Shared by the kernels and a
// host build (scan_host.cpp, loaded only by the CPU tests).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BSHUF_TS_HD __host__ __device__
#else
#define BSHUF_TS_HD
#endif

#ifndef BSHUF_TICKET_SHARDS
#define BSHUF_TICKET_SHARDS 8  // a power of two; A/B builds: 1 = one counter
#endif

namespace bshuf {

constexpr int kTicketShards = BSHUF_TICKET_SHARDS;
static_assert((kTicketShards & (kTicketShards - 1)) == 0, "shards: a power of two");

// Tickets of shard c that name a block below `end`: shard c's ticket t is block
// first + G + kTicketShards * t + c (a launch of G workgroups over blocks
// [first, end), whose first G blocks are taken without a ticket).  0 for a
// shard that owns no block.
BSHUF_TS_HD inline int64_t ticket_limit(int64_t first, int64_t G, int64_t end, int c) {
    const int64_t left = end - (first + G + c);
    return left <= 0 ? 0 : (left + kTicketShards - 1) / kTicketShards;
}

// What a shard has left: its limit minus its counter, which over-draws past
// the limit (every wave's last tickets) and so is clamped.
BSHUF_TS_HD inline uint32_t ticket_remaining(int64_t limit, uint32_t drawn) {
    return (int64_t)drawn >= limit ? 0u : (uint32_t)(limit - (int64_t)drawn);
}

// The shard to steal from: the one with the most tickets left, ties to the
// nearest shard behind `own` (cyclically; own itself comes last), so that
// thieves of different shards spread out.  -1: no shard has any left.
BSHUF_TS_HD inline int ticket_victim(const uint32_t (&remaining)[kTicketShards], int own) {
    // (every index a constant once unrolled: the kernels keep `remaining` in
    // scalar registers, which a computed index would move to memory)
    int best = -1, best_dist = kTicketShards;
    uint32_t most = 0;
    for (int c = 0; c < kTicketShards; c++) {
        const int dist = (c - own - 1) & (kTicketShards - 1);  // own itself: the farthest
        if (remaining[c] > most || (remaining[c] == most && most != 0 && dist < best_dist)) {
            most = remaining[c];
            best = c;
            best_dist = dist;
        }
    }
    return best;
}

}  // namespace bshuf
