// gtx_pass_queue.hpp -- the queues between the alignment passes behind the general one: the state words of a queue, the blocks
// of them a call keeps, the capacities, and the levels of the exact pass' slab.  Plain C++, no HIP: the library's device and
// host code and the emulations (tests/emu, tests/emu_long) read the same numbers.  The push: wave_hip.hpp, queue_push.
#pragma once
#include <cstdint>

namespace gtx
{
// A queue of (read * 2 + orientation) tasks has eight state words, zeroed before the call.  A pass pushes into the queue of the
// pass behind it; that pass' launch takes min(queued, capacity) tasks through the claim cursor.
constexpr uint32_t Q_QUEUED = 0;  // pushes (beyond the capacity: those tasks were dropped)
constexpr uint32_t Q_CURSOR = 1;  // claim cursor of the launch that takes the queue
constexpr uint32_t Q_DROPPED = 3; // pushes that found the queue full
constexpr uint32_t Q_WORDS = 8;   // from one launch's words to the next one's

// The exact pass is three launches -- a small part of the slab per task, a large part, the whole slab -- each with a queue of
// EXACT_TASK_CAP tasks; the last one hands on to a queue of capacity 0 whose count is what even the whole slab could not hold.
constexpr uint32_t EXACT_LAUNCHES = 3;
constexpr uint32_t EXACT_STATE_WORDS = (EXACT_LAUNCHES + 1) * Q_WORDS;
constexpr uint32_t EXACT_TASK_CAP = 1u << 20;
constexpr uint32_t EXACT_PART_SITES = 24;        // variant sites a path has room for while a task has a small part of the slab
constexpr uint32_t EXACT_PART_CANDIDATES = 8256; // ... and walk candidates (128 live sequences x 64 alleles + a round's slack)
constexpr uint32_t EXACT_LARGE_PARTS = 32, EXACT_LARGE_SITES = 64; // the launch between the small parts and the whole slab

// The short reads' block: the HBM-table pass' queue, the wide-site pass' (graphs with a site of more than 64 alleles), the exact pass'
constexpr uint32_t HBM_STATE_WIDE = Q_WORDS, HBM_STATE_EXACT = 2 * Q_WORDS, HBM_STATE_WORDS = 2 * Q_WORDS + EXACT_STATE_WORDS;
constexpr uint32_t WIDE_TASK_CAP = 1u << 20;

// The long reads' block: tier 1 has no queue -- its eight words hold the read cursor and the tasks it took --, then tier 2's exact pass
constexpr uint32_t LONG_READ_CURSOR = 0, LONG_TASKS = 1, LONG_STATE_EXACT = Q_WORDS, LONG_STATE_WORDS = Q_WORDS + EXACT_STATE_WORDS;

// What an exact pass' launches found, from its state words: out[0..2] each launch's queue, out[3] what the last launch handed
// on plus what full queues dropped
inline void exact_pass_counts(uint32_t const * st, uint64_t * out)
{
  out[EXACT_LAUNCHES] = st[EXACT_LAUNCHES * Q_WORDS + Q_QUEUED];
  for (uint32_t k = 0; k < EXACT_LAUNCHES; ++k)
  {
    out[k] = st[k * Q_WORDS + Q_QUEUED];
    out[EXACT_LAUNCHES] += st[k * Q_WORDS + Q_DROPPED];
  }
}
} // namespace gtx
