// What the launch chains (chain.hip) lean on besides kernels: workspace guard bands, the pool of ordering events and the
// per-launch profiler.  Host code only (chain_support.cpp).
#pragma once
#include "common.hpp"

// return a callee's / a HIP call's failure to the caller (the latter as "<what>: <HIP's message>" in vj_last_error())
#define CH(call)                      \
  do {                                \
    if (int _rc = (call)) return _rc; \
  } while (0)
#define HIPCH(call, what)                                    \
  do {                                                       \
    if (hipError_t _e = (call)) return hip_failed(what, _e); \
  } while (0)
int hip_failed(const char* what, hipError_t e);

// ---- guard bands (option ws_guard): a 256-byte gap behind every member of a workspace layout
int64_t guard_gap();                        // bytes of one gap: 256 with the option, else 0
int guard_begin(void* ws, int64_t bytes);   // a chain call is about to lay its layout over [ws, ws + bytes): inspect and forget the older gaps there
int poison_gap(char* p, hipStream_t st);    // fill the gap at p with the pattern (in stream order) and remember it for vj_ws_guard_check

// ---- event pool
hipEvent_t next_event();   // an ordering event of the current device's pool, or nullptr if the pool could not be created
int stream_after(hipStream_t to, hipStream_t from, const char* what);   // `to` waits for everything enqueued so far on `from`

// ---- launch profiler (vj_prof_enable / vj_prof_collect): the scope brackets the launches enqueued on `stream` during its lifetime
struct ProfScope {
  bool on;
  hipEvent_t s, e;
  hipStream_t st;
  int family, tag;   // family: 0 GEMM, 1 attention forward, 2 attention backward; tag: epilogue for GEMMs, head_dim for attention
  double flop;
  int64_t m, n, k;
  ProfScope(hipStream_t stream, int family, double flop, int64_t m, int64_t n, int64_t k, int tag);
  ~ProfScope();
  ProfScope(const ProfScope&) = delete;
  ProfScope& operator=(const ProfScope&) = delete;
};
