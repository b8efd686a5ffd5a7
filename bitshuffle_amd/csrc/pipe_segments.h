// pipe_segments.h -- the segment bounds of the pipelined encode (launch.h,
// encode_pipelined): which blocks each parse launch of a long call covers.
// Shared by the launcher and a host build (scan_host.cpp, loaded only by the
// CPU tests).
#pragma once
#include <stdint.h>

namespace bshuf {

// Schedules, in 32nds of the call's blocks.  kPipeEqual: eight equal segments.
// kPipeTapered: seven eighths, then 1/16, 1/32, 1/32 -- the last segment's
// scan and compaction run behind the last parse with nothing beside them, so a
// short last segment leaves about 1/32 of the compaction exposed, not 1/8.
enum PipeSchedule { kPipeEqual = 0, kPipeTapered = 1, kPipeSchedules = 2 };
constexpr int kPipeSegsMax = 10;  // segments of the longest schedule

inline int pipe_seg_count(int schedule) { return schedule == kPipeTapered ? 10 : 8; }

// Bound i (0 .. pipe_seg_count) of a call of nb blocks: segment i is blocks
// [bound(i), bound(i + 1)).  Monotone, bound(0) = 0, bound(count) = nb; a
// segment is empty only when nb is smaller than the schedule is fine (the
// launcher skips those).  nb < 2^58.
inline int64_t pipe_seg_bound(int64_t nb, int schedule, int i) {
    static const int8_t equal[] = {0, 4, 8, 12, 16, 20, 24, 28, 32};
    static const int8_t tapered[] = {0, 4, 8, 12, 16, 20, 24, 28, 30, 31, 32};
    const int n = pipe_seg_count(schedule);
    if (i <= 0) return 0;
    if (i >= n) return nb;
    const int64_t k = schedule == kPipeTapered ? tapered[i] : equal[i];
    return nb / 32 * k + nb % 32 * k / 32;
}

}  // namespace bshuf
