// Host-only check of merizo_search_amd/csrc/ms_plan.h (TEST INFRASTRUCTURE; built by tests/test_plan_host.py with the host
// compiler, no HIP): prints a fingerprint of every launch plan and workspace layout over a grid of shapes, devices and switches --
// compared line for line with tests/golden/plan_fingerprints.txt, which was recorded from the planning code as it stood before it
// moved into the header -- and checks on the way that every carved region is aligned, disjoint from the others, inside the
// workspace and large enough for what the kernels write into it.  Exit status 1 and a line per finding on stderr otherwise.
//   plan <switches> <cus> <n> <hash>       one line per (switch set, CU count, n): FNV-1a over every field of every ScanPlan and
//                                          PfLayout of the nq x k x image x mode grid
//   total <n> <nq> <sum> <sum>             default switches, 256 CUs: ms_ip_topk_workspace_bytes and
//                                          ms_ip_topk_prefiltered_workspace_bytes, each summed over the k grid
//   setting <name> <default> <unset> <set> one line per switch: the table's default, what an empty environment gives, and what
//                                          NAME=3 alone gives
// --totals: the 256-CU default-switch sizes case by case instead (n nq k bytes prefiltered_bytes), to hold against a built library.
#include <stdio.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "../../merizo_search_amd/csrc/ms_plan.h"

namespace {

const int64_t NS[] = {0, 1, 31, 32, 33, 1000, 65535, 65536, 70000, 200000, 1000000, 4000000, 45625000, 2147483646};
const int NQS[] = {1, 2, 32, 33, 64, 65, 96, 97, 128, 160, 161, 256, 1024, 4096};
const int KS[] = {1, 4, 5, 10, 11, 20, 21, 24, 25, 32, 33, 48, 49, 64, 65, 128};
const int CUS[] = {256, 304};
typedef std::vector<std::pair<const char *, const char *>> Env;
const Env ENVS[] = {
    {},
    {{"MS_LOADER_WAVE", "0"}},
    {{"MS_PREPASS_TILES", "0"}},
    {{"MS_PREPASS_TILES", "5"}, {"MS_SAMPLE_MIN_NQ", "200"}},
    {{"MS_SAMPLE_MIN_NQ", "1"}},
    {{"MS_LIST_SM", "0"}},
    {{"MS_SHARED_BOUND", "0"}},
    {{"MS_PREFILTER", "0"}},
};

MsSettings settings_of(const Env &env) {
    return ms_parse_settings([&env](const char *name) -> const char * {
        for (const auto &e : env)
            if (strcmp(e.first, name) == 0) return e.second;
        return nullptr;
    });
}

struct Hash {
    uint64_t h = 1469598103934665603ull;
    void add(uint64_t v) {
        for (int i = 0; i < 8; ++i) { h ^= (v >> (8 * i)) & 0xFF; h *= 1099511628211ull; }
    }
};

int findings = 0;
void expect(bool ok, const char *what, int64_t n, int nq, int k, int cus) {
    if (ok) return;
    if (++findings <= 20) fprintf(stderr, "FINDING %s: n=%lld nq=%d k=%d cus=%d\n", what, (long long)n, nq, k, cus);
}

// regions in carve order as (offset, bytes their writers need); `end` closes the last one
void check_regions(const std::vector<std::pair<size_t, size_t>> &r, size_t begin, size_t end, int64_t n, int nq, int k, int cus) {
    for (size_t i = 0; i < r.size(); ++i) {
        const size_t next = i + 1 < r.size() ? r[i + 1].first : end;
        expect(r[i].first % 256 == 0, "region not 256-byte aligned", n, nq, k, cus);
        expect(r[i].first >= (i ? r[i - 1].first : begin) && next >= r[i].first, "regions out of order or outside the workspace", n, nq, k, cus);
        expect(next - r[i].first >= r[i].second, "region smaller than what is written into it", n, nq, k, cus);
    }
}

void hash_plan(Hash &h, const ScanPlan &p) {
    const ScanDevPlan &d = p.d;
    for (int v : {d.nq, d.nq_pad, d.n_qtiles, d.qwb, d.n_qgroups, d.n_sgroups, d.n_streams, d.rows_per_stream, d.P, d.grid, p.k_pass, p.kl,
                  p.prepass_tiles, p.qpw, p.list_sm, (int)p.hist_on})
        h.add((uint64_t)(int64_t)v);
    for (size_t v : {p.lds_bytes, p.off_qn, p.off_inv, p.off_part_s, p.off_part_i, p.off_ub_s, p.off_ub_i, p.off_lb_s, p.off_lb_i, p.off_scr_s,
                     p.off_scr_i, p.off_hist, p.off_hstep, p.off_prog, p.total})
        h.add(v);
}

void check_plan(const ScanPlan &p, int64_t n, int nq, int k, int cus) {
    const ScanDevPlan &d = p.d;
    const size_t q = (size_t)d.nq_pad, lists = (size_t)d.P * q * p.k_pass;
    check_regions({{p.off_qn, q * 128 * 4}, {p.off_inv, (size_t)n * 4}, {p.off_part_s, lists * 4}, {p.off_part_i, lists * 4},
                   {p.off_ub_s, q * 4}, {p.off_ub_i, q * 4}, {p.off_lb_s, q * 4}, {p.off_lb_i, q * 4}, {p.off_scr_s, q * p.k_pass * 4},
                   {p.off_scr_i, q * p.k_pass * 8}, {p.off_hist, q * 16 * 4}, {p.off_hstep, q * 4},
                   {p.off_prog, p.qpw > 0 ? (size_t)d.n_streams * 64 : 0}}, 0, p.total, n, nq, k, cus);
    expect(d.nq == nq && d.nq_pad >= nq && d.nq_pad % 32 == 0, "padded queries", n, nq, k, cus);
    expect((int64_t)d.n_streams * d.rows_per_stream >= n && d.rows_per_stream % 32 == 0, "streams do not cover the rows", n, nq, k, cus);
    expect(2 * p.kl >= p.k_pass && p.k_pass <= 64, "list length", n, nq, k, cus);
    if (p.qpw == 0) {      // the host's plan is the plan the device would make for the same batch
        ScanDevPlan c;
        ms_plan_core(n, nq, cus, &c);
        expect(c.nq == d.nq && c.nq_pad == d.nq_pad && c.n_qtiles == d.n_qtiles && c.qwb == d.qwb && c.n_qgroups == d.n_qgroups &&
               c.n_sgroups == d.n_sgroups && c.n_streams == d.n_streams && c.rows_per_stream == d.rows_per_stream && c.P == d.P &&
               c.grid == d.grid, "make_plan differs from ms_plan_core", n, nq, k, cus);
    }
}

void check_layout(const PfLayout &L, int64_t n, int nq, int k, int cus) {
    check_plan(L.exact, n, nq, k, cus);
    if (!L.ok) { expect(L.total == L.exact.total, "unserved layout is not the fp32 search's", n, nq, k, cus); return; }
    check_plan(L.pf, n, nq, L.kp, cus);
    const size_t q = (size_t)(L.pf.d.nq_pad > L.exact.d.nq_pad ? L.pf.d.nq_pad : L.exact.d.nq_pad);
    size_t lists = 0;      // the exact pass decomposes 1 .. nq flagged queries on the device
    for (int qt = 1; qt <= L.exact.d.n_qtiles; ++qt) {
        ScanDevPlan d;
        ms_plan_core(n, qt * 32 < nq ? qt * 32 : nq, cus, &d);
        expect(d.grid <= L.exact_grid_max && d.P <= L.exact_P_max && d.P <= 256, "device plan outside the launch", n, nq, k, cus);
        if ((size_t)d.nq_pad * d.P * L.exact.k_pass > lists) lists = (size_t)d.nq_pad * d.P * L.exact.k_pass;
    }
    const size_t begin = L.pf.total > L.exact.total ? L.pf.total : L.exact.total;
    check_regions({{L.off_as, q * L.kp * 4}, {L.off_ai, q * L.kp * 8}, {L.off_flag, q * 4}, {L.off_qn_c, q * 128 * 4}, {L.off_lb_c, q * 4},
                   {L.off_qlen_c, q * 4}, {L.off_qmap, q * 4}, {L.off_dp, sizeof(ScanDevPlan)}, {L.off_xs, lists * 4}, {L.off_xi, lists * 4}},
                  begin, L.total, n, nq, k, cus);
    expect(L.kp >= k && L.pf.d.P <= 256, "candidate lists", n, nq, k, cus);
}

void hash_layout(Hash &h, const PfLayout &L) {
    for (int v : {(int)L.ok, L.kp, L.exact_grid_max, L.exact_P_max}) h.add((uint64_t)(int64_t)v);
    for (size_t v : {L.off_as, L.off_ai, L.off_flag, L.off_qn_c, L.off_lb_c, L.off_qlen_c, L.off_qmap, L.off_dp, L.off_xs, L.off_xi, L.total}) h.add(v);
    hash_plan(h, L.exact);
    if (L.ok) hash_plan(h, L.pf);
}

std::string show(int v) { return std::to_string(v); }
std::string show(int64_t v) { return std::to_string(v); }
std::string show(double v) { char b[32]; snprintf(b, sizeof(b), "%.6g", v); return b; }

}  // namespace

int main(int argc, char **argv) {
    const MsSettings dflt = settings_of(ENVS[0]);
    if (argc > 1 && strcmp(argv[1], "--totals") == 0) {
        for (int64_t n : NS) for (int nq : NQS) for (int k : KS)
            printf("%lld %d %d %zu %zu\n", (long long)n, nq, k, make_plan(dflt, 256, n, nq, k).total, pf_workspace_bytes(dflt, 256, n, nq, k));
        return 0;
    }
    for (size_t e = 0; e < sizeof(ENVS) / sizeof(ENVS[0]); ++e) {
        const MsSettings s = settings_of(ENVS[e]);
        std::string label = "default";
        for (size_t i = 0; i < ENVS[e].size(); ++i) label = (i ? label + "," : std::string()) + ENVS[e][i].first + "=" + ENVS[e][i].second;
        for (int cus : CUS) for (int64_t n : NS) {
            Hash h;
            for (int nq : NQS) for (int k : KS) {
                const ScanPlan p = make_plan(s, cus, n, nq, k);
                check_plan(p, n, nq, k, cus);
                hash_plan(h, p);
                for (int image = 0; image < 3; ++image) for (int mode : {MS_MODE_IP_PRENORM, MS_MODE_COSINE_UNIT}) {
                    const PfLayout L = pf_layout(s, cus, n, nq, k, mode, image != 0, image == 2 ? MS_PF_F16X2 : MS_PF_BF16X3);
                    check_layout(L, n, nq, k, cus);
                    hash_layout(h, L);
                }
            }
            printf("plan %s %d %lld %016llx\n", label.c_str(), cus, (long long)n, (unsigned long long)h.h);
        }
    }
    for (int64_t n : NS) for (int nq : NQS) {
        size_t a = 0, b = 0;
        for (int k : KS) { a += make_plan(dflt, 256, n, nq, k).total; b += pf_workspace_bytes(dflt, 256, n, nq, k); }
        printf("total %lld %d %zu %zu\n", (long long)n, nq, a, b);
    }
    const MsSettings table;
#define MS_X(type, member, name, d) \
    printf("setting %s %s %s %s\n", name, show(table.member).c_str(), show(dflt.member).c_str(), show(settings_of({{name, "3"}}).member).c_str());
    MS_SETTINGS_TABLE(MS_X)
#undef MS_X
    if (findings) fprintf(stderr, "%d findings\n", findings);
    return findings ? 1 : 0;
}
