// Host-only check of merizo_search_amd/csrc/ms_wsstate.h (TEST INFRASTRUCTURE; built by tests/test_wsstate_host.py with the host
// compiler, no HIP, once with the address + undefined-behaviour sanitizers and once with the thread sanitizer): the per-workspace
// records of the search path, with the three device functions the header declares defined here over calloc and call counters.
// Prints "checks <count>" on stdout; a line per finding on stderr and exit status 1 otherwise.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../../merizo_search_amd/csrc/ms_wsstate.h"

namespace ws = ms_wsstate;

namespace {
thread_local int t_dev = 0;             // HIP's current device is per host thread too
std::atomic<int> n_alloc{0}, n_drain{0};
int n_checks = 0, n_findings = 0;
}  // namespace

int ws::current_device() { return t_dev; }
void *ws::alloc_zeroed(size_t bytes) { ++n_alloc; return calloc(1, bytes); }
bool ws::drain_and_zero(void *block, size_t bytes) { ++n_drain; memset(block, 0, bytes); return true; }

namespace {

#define CHECK(cond) do { ++n_checks; if (!(cond)) { ++n_findings; fprintf(stderr, "%s:%d: %s\n", __func__, __LINE__, #cond); } } while (0)

const void *wsp(int i) { return reinterpret_cast<const void *>((uintptr_t)0x100000 + (uintptr_t)i * 4096); }      // (never dereferenced)

void reset() {
    for (ws::Record &r : ws::g_table.rec) { free(r.block); r = ws::Record{}; }
    ws::g_table.used = 0;
    ws::g_table.clock = 0;
    n_alloc = 0; n_drain = 0; t_dev = 0;
}
ws::Record *find(const void *w, int dev) {
    for (int i = 0; i < ws::g_table.used; ++i)
        if (ws::g_table.rec[i].ws == w && ws::g_table.rec[i].dev == dev) return &ws::g_table.rec[i];
    return nullptr;
}
bool all_zero(const char *p) { for (size_t i = 0; i < ws::BLOCK_BYTES; ++i) if (p[i] != 0) return false; return true; }

void one_record_per_workspace_and_device() {
    reset();
    char *a0 = ws::block(wsp(0));
    CHECK(a0 != nullptr && all_zero(a0));
    CHECK(ws::block(wsp(0)) == a0);
    ws::mark_clean(wsp(0), 5, 6, 7);                // the counters' books are in the same record
    CHECK(ws::g_table.used == 1 && n_alloc == 1);
    t_dev = 1;
    char *a1 = ws::block(wsp(0));
    CHECK(a1 != nullptr && a1 != a0);
    CHECK(ws::g_table.used == 2 && n_alloc == 2);
    CHECK(!ws::take_clean(wsp(0), 5, 6, 7));        // device 1's record was never marked
    t_dev = 0;
    CHECK(ws::block(wsp(0)) == a0);
    CHECK(ws::take_clean(wsp(0), 5, 6, 7));
    ws::mark_clean(wsp(1), 1, 1, 1);                // a record that only keeps the counters' books owns no block
    CHECK(ws::g_table.used == 3 && n_alloc == 2 && find(wsp(1), 0) != nullptr && find(wsp(1), 0)->block == nullptr);
    t_dev = -1;                                     // no current device: none, and nothing is created
    CHECK(ws::block(wsp(2)) == nullptr && ws::g_table.used == 3);
}

void a_full_table_hands_over_the_least_recently_used_record_of_the_device() {
    reset();
    // workspace 0: a block and every kind of state; then the rest of the table, odd ones without a block
    char *b0 = ws::block(wsp(0));
    memset(b0, 0x5A, ws::BLOCK_BYTES);
    ws::commit_tickets(wsp(0), 7);
    ws::mark_clean(wsp(0), 70000, 96, 10);
    for (int i = 0; i < 3; ++i) (void)ws::next_gate_epoch(wsp(0));
    for (int i = 0; i < 2; ++i) (void)ws::next_pace_epoch(wsp(0));
    for (int i = 1; i < ws::CAPACITY; ++i) {
        if (i % 2 == 0) CHECK(ws::block(wsp(i)) != nullptr);
        else ws::mark_clean(wsp(i), 1000 + i, 2, 10);
    }
    CHECK(ws::g_table.used == ws::CAPACITY && n_drain == 0 && n_alloc == ws::CAPACITY / 2);
    // one more: workspace 0's record (it owned a block: one drain, the block zeroed and handed on, everything else starts over)
    const int X = 1000, Y = 1001, Z = 1002, W = 1003;
    char *bx = ws::block(wsp(X));
    CHECK(bx == b0 && all_zero(bx));
    CHECK(n_drain == 1 && n_alloc == ws::CAPACITY / 2 && ws::g_table.used == ws::CAPACITY);
    CHECK(ws::peek_tickets(wsp(X)) == 0u);
    CHECK(!ws::take_clean(wsp(X), 70000, 96, 10));
    CHECK(ws::next_gate_epoch(wsp(X)) == 1u && ws::next_pace_epoch(wsp(X)) == 1u);
    CHECK(find(wsp(0), 0) == nullptr);
    CHECK(!ws::take_clean(wsp(0), 70000, 96, 10) && ws::peek_tickets(wsp(0)) == 0u);      // workspace 0 is unknown now
    CHECK(ws::take_clean(wsp(5), 1005, 2, 10));                                              // the others kept their state (5 is now recent)
    // the next in line is workspace 1, which owned no block: no drain; a record made for the counters gets no block
    ws::mark_clean(wsp(Y), 3, 3, 3);
    CHECK(n_drain == 1 && find(wsp(1), 0) == nullptr && find(wsp(Y), 0) != nullptr && find(wsp(Y), 0)->block == nullptr);
    CHECK(!ws::take_clean(wsp(Y), 1001, 2, 10) && ws::take_clean(wsp(Y), 3, 3, 3));
    // then workspace 2 (a block: a second drain), then workspace 3 (none: no drain, and the new owner's block is allocated)
    char *b2 = find(wsp(2), 0)->block;
    CHECK(ws::block(wsp(Z)) == b2 && n_drain == 2 && n_alloc == ws::CAPACITY / 2);
    CHECK(ws::block(wsp(W)) != nullptr && n_drain == 2 && n_alloc == ws::CAPACITY / 2 + 1 && find(wsp(3), 0) == nullptr);
    CHECK(ws::g_table.used == ws::CAPACITY);
}

void records_of_other_devices_are_never_taken() {
    reset();
    t_dev = 1;
    for (int i = 0; i < ws::CAPACITY; ++i) CHECK(ws::block(wsp(i)) != nullptr);
    t_dev = 0;
    CHECK(ws::block(wsp(500)) == nullptr);                      // "none"
    ws::mark_clean(wsp(500), 1, 2, 3);
    CHECK(!ws::take_clean(wsp(500), 1, 2, 3));                  // the counters count as dirty
    CHECK(ws::peek_tickets(wsp(500)) == 0u && ws::next_gate_epoch(wsp(500)) != 0u && ws::next_pace_epoch(wsp(500)) != 0u);
    CHECK(n_drain == 0 && n_alloc == ws::CAPACITY);
    for (int i = 0; i < ws::CAPACITY; ++i) CHECK(find(wsp(i), 1) != nullptr);
    // one record of device 0 among device 1's: it is the one device 0 takes, however recently it was used
    reset();
    CHECK(ws::block(wsp(0)) != nullptr);
    t_dev = 1;
    for (int i = 1; i < ws::CAPACITY; ++i) CHECK(ws::block(wsp(i)) != nullptr);
    t_dev = 0;
    char *b0 = ws::block(wsp(0));
    CHECK(ws::block(wsp(500)) == b0 && n_drain == 1 && find(wsp(0), 0) == nullptr);
    for (int i = 1; i < ws::CAPACITY; ++i) CHECK(find(wsp(i), 1) != nullptr);
}

void tickets_advance_on_commit_only() {
    reset();
    CHECK(ws::peek_tickets(wsp(0)) == 0u && ws::g_table.used == 0);      // unknown: 0, and peeking creates nothing
    ws::commit_tickets(wsp(0), 5);
    CHECK(ws::g_table.used == 0);
    (void)ws::block(wsp(0));
    CHECK(ws::peek_tickets(wsp(0)) == 0u && ws::peek_tickets(wsp(0)) == 0u);
    ws::commit_tickets(wsp(0), 96);
    CHECK(ws::peek_tickets(wsp(0)) == 96u);
    // a call that fails between peek and commit: the next one sees the same base
    const uint32_t base = ws::peek_tickets(wsp(0));
    (void)ws::next_gate_epoch(wsp(0));
    CHECK(ws::peek_tickets(wsp(0)) == base);
    ws::commit_tickets(wsp(0), 0xFFFFFFF0u - 96u);
    CHECK(ws::peek_tickets(wsp(0)) == 0xFFFFFFF0u);
    ws::commit_tickets(wsp(0), 0x20u);                                    // across 2^32, as the device word
    CHECK(ws::peek_tickets(wsp(0)) == 0x10u);
    (void)ws::block(wsp(1));
    CHECK(ws::peek_tickets(wsp(1)) == 0u);                                // per workspace
}

void counters_are_clean_once_per_mark_and_shape() {
    reset();
    CHECK(!ws::take_clean(wsp(0), 70000, 96, 10) && ws::g_table.used == 0);      // unknown workspace
    ws::invalidate(wsp(0));
    CHECK(ws::g_table.used == 0);
    ws::mark_clean(wsp(0), 70000, 96, 10);
    CHECK(!ws::take_clean(wsp(0), 70001, 96, 10) && !ws::take_clean(wsp(0), 70000, 64, 10) && !ws::take_clean(wsp(0), 70000, 96, 7));
    CHECK(!ws::take_clean(wsp(1), 70000, 96, 10));
    CHECK(ws::take_clean(wsp(0), 70000, 96, 10));
    CHECK(!ws::take_clean(wsp(0), 70000, 96, 10));
    ws::mark_clean(wsp(0), 70000, 96, 10);
    ws::invalidate(wsp(0));
    CHECK(!ws::take_clean(wsp(0), 70000, 96, 10));
    ws::mark_clean(wsp(0), 70000, 96, 10);
    ws::mark_clean(wsp(0), 777, 2, 10);                                           // the last mark's shape holds
    CHECK(!ws::take_clean(wsp(0), 70000, 96, 10) && ws::take_clean(wsp(0), 777, 2, 10));
}

void epochs_are_never_zero() {
    reset();
    (void)ws::block(wsp(0));
    (void)ws::block(wsp(1));
    CHECK(ws::next_gate_epoch(wsp(0)) == 1u && ws::next_gate_epoch(wsp(0)) == 2u && ws::next_gate_epoch(wsp(1)) == 1u);
    find(wsp(0), 0)->gate_epoch = 0xFFFFFFFDu;
    const uint32_t want[] = {0xFFFFFFFEu, 0xFFFFFFFFu, 1u, 2u, 3u};
    for (uint32_t w : want) CHECK(ws::next_gate_epoch(wsp(0)) == w);
    CHECK(ws::next_gate_epoch(wsp(1)) == 2u);
    uint32_t prev = 0;
    for (int i = 0; i < 600; ++i) {
        const uint32_t e = ws::next_pace_epoch(wsp(0));
        CHECK(e >= 1u && e <= 255u && e != prev);
        if (i == 2) CHECK(ws::next_pace_epoch(wsp(1)) == 1u);       // another workspace draws on its own
        prev = e;
    }
    CHECK(prev == (600u - 1u) % 255u + 1u && ws::next_pace_epoch(wsp(1)) == 2u);
}

struct Tally { uint32_t tickets = 0, gate = 0, pace = 0; int marked = 0, taken = 0; };
void worker(const void *w, int salt, Tally *t) {
    (void)ws::block(w);
    for (int i = 0; i < 10000; ++i) {
        switch ((i + salt) % 7) {
        case 0: (void)ws::block(w); break;
        case 1: ws::mark_clean(w, 70000, 96, 10); ++t->marked; break;
        case 2: t->taken += ws::take_clean(w, 70000, 96, 10) ? 1 : 0; break;
        case 3: (void)ws::peek_tickets(w); break;
        case 4: ws::commit_tickets(w, (uint32_t)i * 2654435761u); t->tickets += (uint32_t)i * 2654435761u; break;
        case 5: if (ws::next_gate_epoch(w) == 0u) t->gate += 1u << 31; ++t->gate; break;
        default: { const uint32_t e = ws::next_pace_epoch(w); if (e < 1u || e > 255u) t->pace += 1u << 31; ++t->pace; }
        }
    }
}
void threads_keep_the_totals() {
    reset();
    Tally tally[10];
    std::vector<std::thread> th;
    for (int i = 0; i < 10; ++i) th.emplace_back(worker, wsp(i < 8 ? i : 8), i, &tally[i]);       // 8 on their own workspace, 2 share one
    for (std::thread &t : th) t.join();
    tally[8].tickets += tally[9].tickets; tally[8].gate += tally[9].gate; tally[8].pace += tally[9].pace;
    tally[8].marked += tally[9].marked; tally[8].taken += tally[9].taken;
    CHECK(ws::g_table.used == 9 && n_alloc == 9 && n_drain == 0);
    for (int i = 0; i < 9; ++i) {
        const ws::Record *r = find(wsp(i), 0);
        CHECK(r != nullptr);
        if (r == nullptr) continue;
        CHECK(ws::peek_tickets(wsp(i)) == tally[i].tickets);
        CHECK(tally[i].gate < (1u << 31) && r->gate_epoch == tally[i].gate);
        CHECK(tally[i].pace < (1u << 31) && r->pace_epoch == (tally[i].pace - 1u) % 255u + 1u);
        // every mark is taken at most once; a thread alone on its workspace takes each of its marks (the take follows the mark)
        CHECK(tally[i].taken <= tally[i].marked && (i == 8 || tally[i].marked - tally[i].taken <= 1));
    }
}

}  // namespace

int main() {
    static_assert(ws::CAPACITY >= 80 && ws::CAPACITY <= 128, "room for what the two old tables held (64 + 16), and no more than 128");
    one_record_per_workspace_and_device();
    a_full_table_hands_over_the_least_recently_used_record_of_the_device();
    records_of_other_devices_are_never_taken();
    tickets_advance_on_commit_only();
    counters_are_clean_once_per_mark_and_shape();
    epochs_are_never_zero();
    threads_keep_the_totals();
    reset();
    printf("checks %d\n", n_checks);
    return n_findings == 0 ? 0 : 1;
}
