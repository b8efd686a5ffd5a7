// Host build of the decoder's scan state machine (lz4_scan.h), of the
// ticket-stealing arithmetic (ticket_steal.h) and of the pipelined encode's
// segment bounds (pipe_segments.h) for the CPU test suite.  Not part of the
// product library.
#include <stdint.h>

#include "lz4_scan.h"
#include "pipe_segments.h"
#include "ticket_steal.h"

namespace {
struct HostReader {
    const uint8_t* P;
    uint32_t operator()(int p) const { return P[p]; }
};
struct HostOut {
    uint32_t* pos;
    void put(int i, uint32_t v, int op) {
        pos[i] = v;
        (void)op;
    }
};
}  // namespace

extern "C" int bshuf_hostcheck_scan(const uint8_t* payload, int clen, int n, uint32_t* pos,
                                    int* nseq) {
    HostReader rd{payload};
    HostOut out{pos};
    int cnt = 0;
    const int r = bshuf::scan_block(rd, clen, n, out, cnt);
    *nseq = cnt;
    return r;
}

// pipe_segments.h as the launcher uses it
extern "C" int bshuf_hostcheck_pipe_schedules(void) { return bshuf::kPipeSchedules; }
extern "C" int bshuf_hostcheck_pipe_segs_max(void) { return bshuf::kPipeSegsMax; }
extern "C" int bshuf_hostcheck_pipe_seg_count(int schedule) { return bshuf::pipe_seg_count(schedule); }
extern "C" int64_t bshuf_hostcheck_pipe_seg_bound(int64_t nb, int schedule, int i) {
    return bshuf::pipe_seg_bound(nb, schedule, i);
}

// ticket_steal.h as the kernels use it
extern "C" int bshuf_hostcheck_ticket_shards(void) { return bshuf::kTicketShards; }
extern "C" int64_t bshuf_hostcheck_ticket_limit(int64_t first, int64_t G, int64_t end, int shard) {
    return bshuf::ticket_limit(first, G, end, shard);
}
extern "C" uint32_t bshuf_hostcheck_ticket_remaining(int64_t limit, uint32_t drawn) {
    return bshuf::ticket_remaining(limit, drawn);
}
// remaining: kTicketShards words
extern "C" int bshuf_hostcheck_ticket_victim(const uint32_t* remaining, int own) {
    uint32_t r[bshuf::kTicketShards];
    for (int c = 0; c < bshuf::kTicketShards; c++) r[c] = remaining[c];
    return bshuf::ticket_victim(r, own);
}
