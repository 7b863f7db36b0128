// What the host remembers about a search workspace between calls: ONE record per (workspace pointer, device ordinal), in one fixed table
// under one mutex.  Plain C++17, no HIP include (as ms_plan.h): tests/c_abi/wsstate_check.cpp exercises it on a CPU.  When the table is
// full, the least recently used record OF THE CALLER'S DEVICE changes hands: the device drains first (launches of the old workspace may
// still be in flight on another stream) and the block is zeroed again; ticket total, clean flag and epochs start over with it.  Records of
// other devices are never taken: with none of its own a caller gets "none" and does without (ms_ip_topk runs the unfused merge, a
// prefiltered search takes the fp32 path, the counters count as dirty).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <mutex>
#include <utility>
namespace ms_wsstate {
// The device, as far as this header needs it: declared here, defined by whoever includes it (ms_search.hip: HIP; the test: calloc)
int current_device();                               // ordinal of the calling thread's current device; < 0: unknown
void *alloc_zeroed(size_t bytes);                   // device memory, zeroed; nullptr: none to be had
bool drain_and_zero(void *block, size_t bytes);     // wait for all work queued on the current device, then zero the block again
constexpr int CAPACITY = 96;            // (the two tables this one replaces held 64 blocks and 16 counter records)
constexpr size_t BLOCK_BYTES = 512;     // [0,256) the 64 arrival counters of the in-launch merge, which every launch leaves zero again;
constexpr size_t GATE_OFFSET = 256;     // +256 the prefilter's gate words: [0] gate, [1] epoch, [2] flagged count, [4] slot counter, [5] ticket
struct Record {
    const void *ws = nullptr; int dev = 0;      // the key
    // Device memory the library allocates and zeroes itself on first need (a record that only keeps the counters' books owns none), not the caller's
    // workspace: a freed workspace's address may come back holding anything.  Calls that share a workspace are serialised by the caller, so they share it.
    char *block = nullptr;
    uint64_t last_use = 0;
    uint32_t tickets = 0;       // running total of the compaction's ticket = the value of the device's ticket word, which is never reset
    // Are the shared bound's histogram counters (ScanHist) still zero, as ms_sample_bound_kernel left them for a scan of this shape?  Every
    // scan needs them zero; one that cannot take them for clean zeroes them itself, so this is only an optimisation's bookkeeping.
    int64_t n = 0;
    int nq = 0, k = 0;
    bool clean = false;
    uint32_t gate_epoch = 0;    // the last one handed out; never 0 (a zeroed gate word)
    uint32_t pace_epoch = 0;    // likewise, 1..255: the image scans keep it in the top byte of a progress word, and a zeroed word has 0
};
struct Table { std::mutex mutex; Record rec[CAPACITY]; int used = 0; uint64_t clock = 0; };      // (the mutex guards the rest)
inline Table g_table;
enum Want { FIND, CREATE, CREATE_WITH_BLOCK };
// (the caller holds the mutex) -> the record of (ws, current device), or nullptr: unknown (FIND), or none to be had
inline Record *record_locked(Table &t, const void *ws, Want want) {
    const int dev = current_device();
    Record *r = nullptr, *lru = nullptr;
    for (Record *e = t.rec; e < t.rec + t.used && r == nullptr; ++e)
        if (e->dev == dev && e->ws == ws) r = e;
        else if (e->dev == dev && (lru == nullptr || e->last_use < lru->last_use)) lru = e;
    if (r == nullptr) {
        if (want == FIND || dev < 0) return nullptr;
        if (t.used < CAPACITY) lru = &t.rec[t.used++];
        else if (lru == nullptr || (lru->block != nullptr && !drain_and_zero(lru->block, BLOCK_BYTES))) return nullptr;
        r = lru;
        *r = Record{ws, dev, r->block};         // (everything else starts over)
    }
    if (want == CREATE_WITH_BLOCK && r->block == nullptr && (r->block = static_cast<char *>(alloc_zeroed(BLOCK_BYTES))) == nullptr) return nullptr;
    r->last_use = ++t.clock;
    return r;
}
// One lock acquisition, one look-up: every operation below is one of these
struct Locked { std::lock_guard<std::mutex> lock{g_table.mutex}; Record *r; Locked(const void *ws, Want want) : r(record_locked(g_table, ws, want)) {} };
inline char *block(const void *ws) { Locked l(ws, CREATE_WITH_BLOCK); return l.r != nullptr ? l.r->block : nullptr; }      // nullptr: none
// Counters: a sample pass of this shape just zeroed them / were they clean for this shape? (dirty afterwards) / a scan ran outside the staged bookkeeping
inline void mark_clean(const void *ws, int64_t n, int nq, int k) { Locked l(ws, CREATE); if (l.r != nullptr) { l.r->n = n; l.r->nq = nq; l.r->k = k; l.r->clean = true; } }
inline bool take_clean(const void *ws, int64_t n, int nq, int k) { Locked l(ws, FIND); return l.r != nullptr && l.r->n == n && l.r->nq == nq && l.r->k == k && std::exchange(l.r->clean, false); }
inline void invalidate(const void *ws) { Locked l(ws, FIND); if (l.r != nullptr) l.r->clean = false; }
// Tickets: the value the first arrival of the next re-scoring launch will see / that launch is enqueued, the device word advances by `count` (modulo 2^32)
inline uint32_t peek_tickets(const void *ws) { Locked l(ws, FIND); return l.r != nullptr ? l.r->tickets : 0u; }
inline void commit_tickets(const void *ws, uint32_t count) { Locked l(ws, FIND); if (l.r != nullptr) l.r->tickets += count; }
// Epochs: 1, 2, ... 2^32 - 1, 1, ... and 1, 2, ... 255, 1, ...
inline uint32_t next_gate_epoch(const void *ws) { Locked l(ws, FIND); return l.r == nullptr ? 1u : (++l.r->gate_epoch != 0u ? l.r->gate_epoch : ++l.r->gate_epoch); }
inline uint32_t next_pace_epoch(const void *ws) { Locked l(ws, FIND); return l.r == nullptr ? 1u : (l.r->pace_epoch = l.r->pace_epoch % 255u + 1u); }
}  // namespace ms_wsstate
