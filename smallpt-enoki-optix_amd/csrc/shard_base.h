// shard_base.h — the segments of a sharded queue (spt_internal.h includes it;
// host-only code defines SPT_HD itself, tests/native/shard_base_check.cpp).
#pragma once
#include <stdint.h>

namespace spt {

// A queue filled by a sharded producer (camera_cast_kernel): survivors of
// block b go to shard b mod kShards — the XCD the block runs on — through
// that shard's own counter, into segment [shard_base(j), shard_base(j) +
// count_j) of the queue.  One queue counter takes at most ~88 atomics per us
// (MI355X_MICROARCH.md, dequeue), so a first cast of 67M paths in 262144
// blocks on one counter waited ~3 ms for its compaction atomics; eight
// counters (and the drain's per-XCD pools over the same segments) take
// eight times that.  Segment j holds as many slots as shard j has threads.
constexpr uint32_t kShards = 8;
constexpr uint32_t kShardStride = 32;  // words between shard counters (one 128-B line each)
SPT_HD uint32_t shard_base(uint32_t j, uint32_t items, uint32_t block) {
    const uint32_t nb = (items + block - 1) / block;
    uint32_t base = 0;
    for (uint32_t i = 0; i < j; i++) {
        if (i >= nb) break;
        base += ((nb - 1 - i) / kShards + 1) * block;  // blocks i, i + 8, ... of `block` threads
        if ((nb - 1) % kShards == i) base -= nb * block - items;  // the last block is short
    }
    return base;
}

}  // namespace spt
