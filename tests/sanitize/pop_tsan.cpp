// pop_tsan.cpp -- TEST INFRASTRUCTURE (tests/test_pop_tsan.py).  The
// pipelined run's pop protocol under ThreadSanitizer: 16 threads stand in for
// workgroups and run the functions pop_task itself calls (hl_sched.h: key,
// choice, head rule, slot / claim / head transitions) with task_deps /
// task_succ (hl_pipeline.h) over a run of four 8 x 3-MB pictures whose tasks
// cost nothing.  Every scheduler word is a std::atomic; each task writes a
// plain payload word that its successors read after their pop, so the
// release of a push and the acquire of a pop are what keeps the run free of
// races.  End state: every task ran exactly once, every head equals its
// tail, every pushed slot is taken.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../hartallo_amd/csrc/hl_pipeline.h"

namespace {
constexpr int kThreads = 16, kMbw = 8, kMbh = 3, kNf = 4, kR = 2, kSubQ = 4, kHop = 18;
constexpr int kNmb = kMbw * kMbh, kTasks = kNf * kNmb, kQueues = kNf * kSubQ;

std::atomic<int32_t> g_queue[kQueues * kNmb + 4], g_head[kQueues], g_tail[kQueues], g_claim[kTasks], g_cnt[kTasks], g_poppers, g_done;
std::atomic<int32_t> g_ran[kTasks];
int32_t g_payload[kTasks];  // plain: written by the task, read by its successors
std::atomic<long> g_lost, g_bad, g_shared;  // (g_shared: tasks of threads other than the run's busiest)
std::atomic<int> g_go;  // the threads of a run start together

int32_t* word(std::atomic<int32_t>* a) { return reinterpret_cast<int32_t*>(a); }

// one task: its dependencies' payloads, its own, then its successors (k_pipeline's release)
void run_task(int t)
{
    const int f = t / kNmb, a = t % kNmb, x = a % kMbw, y = a / kMbw;
    g_ran[t].fetch_add(1, std::memory_order_relaxed);
    int d[3][3];
    const int nd = hl::task_deps(f, x, y, kMbw, kMbh, kR, d);
    int32_t sum = 1;
    for (int i = 0; i < nd; ++i) {
        const int32_t p = g_payload[d[i][0] * kNmb + d[i][2] * kMbw + d[i][1]];
        if (p <= 0) g_bad.fetch_add(1);
        sum += p & 0xffff;
    }
    g_payload[t] = sum;
    int fo = 0, xo = 0, yo = 0;
    const int ns = hl::task_succ(f, x, y, kMbw, kMbh, kR, kNf, -1, fo, xo, yo);
    for (int j = 0; j < ns; ++j) {
        hl::task_succ(f, x, y, kMbw, kMbh, kR, kNf, j, fo, xo, yo);
        const int s = fo * kNmb + yo * kMbw + xo;
        if (g_cnt[s].fetch_sub(1, std::memory_order_acq_rel) != 1) continue;
        const int q = fo * kSubQ + xo * kSubQ / kMbw;
        const int pos = g_tail[q].fetch_add(1, std::memory_order_relaxed);
        g_queue[q * kNmb + pos].store(yo * kMbw + xo + 1, std::memory_order_release);
    }
    g_done.fetch_add(1, std::memory_order_release);
}

// pop_task's round, a lane per queue; -1 once the run has finished
int pop(int w)
{
    uint32_t seq = (uint32_t)w;
    int stood_back = 0;
    g_poppers.fetch_add(1, std::memory_order_relaxed);
    for (;;) {
        const int poppers = g_poppers.load(std::memory_order_relaxed);
        int hs[kQueues], ts[kQueues], p0[kQueues], packed[kQueues][hl::kPopLook], lbest[kQueues], bidx[kQueues];
        int32_t qv[kQueues][hl::kPopLook];
        for (int q = 0; q < kQueues; ++q) {
            hs[q] = g_head[q].load(std::memory_order_relaxed);
            ts[q] = g_tail[q].load(std::memory_order_relaxed);
        }
        int best = -1;
        for (int q = 0; q < kQueues; ++q) {
            const int g = (q * kNmb + hs[q]) & ~(hl::kPopLook - 1);
            p0[q] = g - q * kNmb;
            lbest[q] = -1;
            bidx[q] = 0;
            for (int s = 0; s < hl::kPopLook; ++s) {
                const int p = p0[q] + s;
                qv[q][s] = hs[q] < ts[q] && p >= hs[q] && p < ts[q] ? g_queue[g + s].load(std::memory_order_relaxed) : 0;
                packed[q][s] = -1;
                if (qv[q][s] > 0) {
                    const int a = qv[q][s] - 1;
                    packed[q][s] = hl::sched_pack(hl::sched_key(kMbw, kMbh, a % kMbw, a / kMbw, kHop, q / kSubQ, q % kSubQ == w % kSubQ ? 30 : 0), q);
                    if (packed[q][s] > lbest[q]) lbest[q] = packed[q][s], bidx[q] = s;
                }
            }
            const int to = hl::sched_head_target(hs[q], ts[q], p0[q], qv[q], hl::kPopLook, -1);
            if (to > hs[q]) hl::sched_advance_head(word(g_head + q), to);
            if (lbest[q] > best) best = lbest[q];
        }
        if (best < 0) {
            if (g_done.load(std::memory_order_acquire) == kTasks) {
                g_poppers.fetch_sub(1, std::memory_order_relaxed);
                return -1;
            }
            std::this_thread::yield();
            continue;
        }
        uint64_t within = 0;
        for (int q = 0; q < kQueues; ++q)
            if (hl::sched_within(lbest[q], best, hl::kPopSpread)) within |= 1ull << q;
        const int m = hl::sched_spread_count(within, poppers);
        const int q = hl::sched_choose(within, hl::sched_packed_lane(best), seq, poppers, stood_back >= hl::kPopStandBack);
        if (q < 0) {  // more poppers than entries: this one stands back for a round
            ++stood_back;
            seq = hl::sched_seq_next(seq);
            std::this_thread::yield();
            continue;
        }
        stood_back = 0;
        int s = bidx[q];
        if (m > 1) {
            int c = 0;
            for (int i = 0; i < hl::kPopLook; ++i) c += hl::sched_within(packed[q][i], best, hl::kPopSpread) ? 1 : 0;
            int rth = hl::sched_in_lane(seq, m, c > 1 ? c : 1);
            for (int i = 0; i < hl::kPopLook; ++i)
                if (hl::sched_within(packed[q][i], best, hl::kPopSpread) && rth-- == 0) s = i;
        }
        const int32_t v = qv[q][s];
        const int pos = p0[q] + s;
        if (hl::sched_take_slot(word(g_queue + q * kNmb + pos), v)) {
            const int t = (q / kSubQ) * kNmb + v - 1;
            const bool got = hl::sched_claim_task(word(g_claim + t));
            const int to = hl::sched_head_target(hs[q], ts[q], p0[q], qv[q], hl::kPopLook, pos);
            if (to > hs[q]) hl::sched_advance_head(word(g_head + q), to);
            if (got) {
                g_poppers.fetch_sub(1, std::memory_order_relaxed);
                return t;
            }
        }
        g_lost.fetch_add(1, std::memory_order_relaxed);
        seq = hl::sched_seq_next(seq);
    }
}
}  // namespace

int main()
{
    for (int rep = 0; rep < 8; ++rep) {
        for (auto& w : g_queue) w.store(0);
        for (int q = 0; q < kQueues; ++q) g_head[q].store(0), g_tail[q].store(0);
        for (int t = 0; t < kTasks; ++t) {
            int d[3][3];
            g_cnt[t].store(hl::task_deps(t / kNmb, t % kNmb % kMbw, t % kNmb / kMbw, kMbw, kMbh, kR, d));
            g_claim[t].store(0);
            g_ran[t].store(0);
            g_payload[t] = 0;
        }
        g_poppers.store(0);
        g_done.store(0);
        g_queue[0].store(1);
        g_tail[0].store(1);
        std::vector<std::thread> th;
        int per[kThreads] = {};
        for (int w = 0; w < kThreads; ++w)
            th.emplace_back([w, rep, &per] {
                while (g_go.load(std::memory_order_acquire) != rep + 1) {
                }
                for (int t; (t = pop(w)) >= 0; ++per[w]) run_task(t);
            });
        g_go.store(rep + 1, std::memory_order_release);
        for (auto& t : th) t.join();
        int most = 0;
        for (int w = 0; w < kThreads; ++w) most = per[w] > most ? per[w] : most;
        g_shared.fetch_add(kTasks - most);
        int bad = (int)g_bad.load();
        for (int t = 0; t < kTasks; ++t) bad += g_ran[t].load() != 1;
        for (int q = 0; q < kQueues; ++q) {
            bad += g_head[q].load() != g_tail[q].load();
            for (int p = 0; p < g_tail[q].load(); ++p) bad += g_queue[q * kNmb + p].load() >= 0;
        }
        bad += g_poppers.load() != 0;
        if (bad) {
            printf("pop_tsan: run %d: %d end-state checks failed\n", rep, bad);
            return 1;
        }
    }
    printf("pop ok: 8 runs of %d tasks on %d threads, %ld lost attempts, %ld tasks run beside each run's busiest thread\n", kTasks, kThreads,
           g_lost.load(), g_shared.load());
    return 0;
}
