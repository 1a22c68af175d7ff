// Support code of the launch chains (chain.hip), host only: the workspace guard bands, the pool of ordering events and the
// per-launch profiler behind vj_ws_guard_check / vj_prof_enable / vj_prof_collect.
#include "chain_support.hpp"
#include "options.hpp"
#include "../../include/vjepa_hip.h"
#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

int hip_failed(const char* what, hipError_t e) {
  vj_set_error("%s: %s", what, hipGetErrorString(e));
  return (int)e;
}

// ---------------------------------------------------------------------------------------------------- guard bands
// Option ws_guard (diagnostics, tests/test_chain_gpu.py): every member of the two workspace layouts is followed by a 256-byte
// gap.  A chain call fills the gaps of the workspace it was given with a byte pattern (in stream order, before its first
// kernel) and remembers where they are; vj_ws_guard_check() synchronises the device and counts the gaps whose pattern
// changed -- a kernel that writes past the end of a saved activation, a column-partial or a split-K buffer lands in one.
#define GUARD_BYTES 256
#define GUARD_PATTERN 0xA5
namespace {
std::mutex g_guard_mu;
std::vector<char*> g_guards;   // device addresses of the gaps poisoned and not yet inspected
int64_t g_guard_checked = 0, g_guard_bad = 0;
char* g_guard_first_bad = nullptr;

// inspect (and forget) the recorded gaps inside [lo, hi); the device must be idle.  Caller holds g_guard_mu.
int inspect_gaps(char* lo, char* hi) {
  std::sort(g_guards.begin(), g_guards.end());
  g_guards.erase(std::unique(g_guards.begin(), g_guards.end()), g_guards.end());
  std::vector<char*> keep;
  unsigned char host[GUARD_BYTES];
  for (char* p : g_guards) {
    if (p < lo || p >= hi) {
      keep.push_back(p);
      continue;
    }
    HIPCH(hipMemcpy(host, p, GUARD_BYTES, hipMemcpyDeviceToHost), "ws_guard");
    bool bad = false;
    for (int i = 0; i < GUARD_BYTES; i++) bad |= host[i] != GUARD_PATTERN;
    g_guard_checked++;
    if (bad) {
      if (g_guard_bad == 0) g_guard_first_bad = p;
      g_guard_bad++;
    }
  }
  g_guards.swap(keep);
  return 0;
}
}  // namespace

int64_t guard_gap() { return vj_opt(VJ_OPT_WS_GUARD) ? GUARD_BYTES : 0; }

// A chain call is about to lay ITS members (and gaps) over [ws, ws + bytes): gaps recorded there by earlier calls belong to an
// older layout (another trunk sharing the temporary workspace, other sequence lengths) and are about to be overwritten
// legitimately -- inspect them now (device-wide synchronise: this is a diagnostic mode), then forget them.
int guard_begin(void* ws, int64_t bytes) {
  std::lock_guard<std::mutex> lk(g_guard_mu);
  bool any = false;
  for (char* p : g_guards) any |= (p >= (char*)ws && p < (char*)ws + bytes);
  if (!any) return 0;
  HIPCH(hipDeviceSynchronize(), "ws_guard");
  return inspect_gaps((char*)ws, (char*)ws + bytes);
}

int poison_gap(char* p, hipStream_t st) {
  HIPCH(hipMemsetAsync(p, GUARD_PATTERN, GUARD_BYTES, st), "ws_guard: hipMemsetAsync failed");
  std::lock_guard<std::mutex> lk(g_guard_mu);
  g_guards.push_back(p);
  return 0;
}

// -> gaps inspected since the last call in *n_checked, those that no longer held the pattern in *n_bad; synchronises the device,
// inspects every gap still recorded and resets the counters
extern "C" int vj_ws_guard_check(int64_t* n_checked, int64_t* n_bad) {
  VJ_CHECK_ARG(n_checked != nullptr && n_bad != nullptr, "vj_ws_guard_check: null output");
  HIPCH(hipDeviceSynchronize(), "vj_ws_guard_check");
  std::lock_guard<std::mutex> lk(g_guard_mu);
  if (int rc = inspect_gaps(nullptr, (char*)UINTPTR_MAX)) return rc;
  *n_checked = g_guard_checked;
  *n_bad = g_guard_bad;
  if (g_guard_bad) vj_set_error("vj_ws_guard_check: %ld damaged gaps, the first at device address %p", (long)g_guard_bad, (void*)g_guard_first_bad);
  g_guard_checked = g_guard_bad = 0;
  g_guard_first_bad = nullptr;
  return 0;
}

// ---------------------------------------------------------------------------------------------------- event pool
// Ordering events (no timing) reused round-robin: hipStreamWaitEvent captures the record that precedes it at call time,
// so an event may be re-recorded as soon as its wait has been enqueued, which always happens inside the same chain call.
namespace {
constexpr int POOL = 1024;
struct EventPool {   // one per device: an event belongs to the device that was current when it was created
  hipEvent_t ev[POOL];
  std::once_flag once;
  std::atomic<unsigned> next{0};
  bool ok = false;
};
EventPool g_pools[VJ_MAX_DEVICES];
}  // namespace

hipEvent_t next_event() {
  EventPool& P = g_pools[vj_device_slot()];
  std::call_once(P.once, [&P] {
    P.ok = true;
    for (int i = 0; i < POOL; i++)
      if (hipEventCreateWithFlags(&P.ev[i], hipEventDisableTiming) != hipSuccess) P.ok = false;
  });
  return P.ok ? P.ev[P.next.fetch_add(1) % POOL] : nullptr;
}

int stream_after(hipStream_t to, hipStream_t from, const char* what) {
  hipEvent_t e = next_event();
  if (e == nullptr) {
    vj_set_error("%s: could not create ordering events", what);
    return -2;
  }
  HIPCH(hipEventRecord(e, from), what);
  HIPCH(hipStreamWaitEvent(to, e, 0), what);
  return 0;
}

// ---------------------------------------------------------------------------------------------------- profiler
// bench.py's roofline object needs per-launch durations of the dominant kernels measured with HIP events on the
// launch stream.  Off by default (no event is created or recorded); vj_prof_enable(1) starts collecting.
namespace {
struct ProfRec {   // a finished ProfScope
  hipEvent_t s, e;
  int family, tag;
  double flop;
  int64_t m, n, k;
};
std::mutex g_prof_mu;
std::vector<ProfRec> g_prof;
std::atomic<int> g_prof_on{0};
}  // namespace

ProfScope::ProfScope(hipStream_t stream, int fam, double fl, int64_t M, int64_t N, int64_t K, int tg)
    : on(g_prof_on.load() != 0), st(stream), family(fam), tag(tg), flop(fl), m(M), n(N), k(K) {
  if (!on) return;
  if (hipEventCreate(&s) != hipSuccess || hipEventCreate(&e) != hipSuccess) {
    on = false;
    return;
  }
  (void)hipEventRecord(s, st);
}
ProfScope::~ProfScope() {
  if (!on) return;
  (void)hipEventRecord(e, st);
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof.push_back({s, e, family, tag, flop, m, n, k});
}

extern "C" int vj_prof_enable(int on) {
  g_prof_on.store(on ? 1 : 0);
  return 0;
}

// Sums per family: ms[3], flop[3], launches[3]; optional CSV of every launch (family,tag,m,n,k,us) at csv_path.
// Synchronises the recorded events (call after the work has been enqueued); clears the records.
extern "C" int vj_prof_collect(double* ms, double* flop, int64_t* launches, const char* csv_path) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (int i = 0; i < 3; i++) {
    ms[i] = 0.0;
    flop[i] = 0.0;
    launches[i] = 0;
  }
  FILE* f = csv_path && csv_path[0] ? fopen(csv_path, "w") : nullptr;
  if (f) fprintf(f, "family,tag,m,n,k,us,flop\n");
  for (auto& r : g_prof) {
    float t = 0.f;
    HIPCH(hipEventSynchronize(r.e), "vj_prof_collect");
    HIPCH(hipEventElapsedTime(&t, r.s, r.e), "vj_prof_collect");
    ms[r.family] += t;
    flop[r.family] += r.flop;
    launches[r.family] += 1;
    if (f) fprintf(f, "%d,%d,%ld,%ld,%ld,%.3f,%.6e\n", r.family, r.tag, (long)r.m, (long)r.n, (long)r.k, 1e3 * t, r.flop);
    (void)hipEventDestroy(r.s);
    (void)hipEventDestroy(r.e);
  }
  if (f) fclose(f);
  g_prof.clear();
  return 0;
}
