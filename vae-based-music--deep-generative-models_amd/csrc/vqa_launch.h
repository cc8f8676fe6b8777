// vqa_launch.h — host-side launch support shared by every translation unit of libvqa (the functions declared here
// are defined in vqa_runtime.hip).
//
// One policy for the HIP calls that configure a kernel instead of launching it: each is cached, so it runs during
// the eager warm-up and never inside a hipGraph capture (a captured step replays launches only).
#pragma once
#include "vqa_common.h"

namespace vqa {

// Multiprocessor count of the current device, queried once. 256 when the query fails (no device: the host-only
// workspace and route queries still answer).
int cu_count();

// Raise fn's dynamic-LDS limit when a launch needs more than the 64 KiB default; the value is the exact need (static
// LDS counts against the 160 KiB too). A per-kernel high-water mark: the attribute is set only when `bytes` exceeds
// what fn already has. VQA_E_UNSUPPORTED (error text "<what>: cannot reserve ...") when the device refuses.
int raise_dyn_lds(const void* fn, size_t bytes, const char* what);

// Resident workgroups of fn per CU at this block size and dynamic LDS (the occupancy API: VGPR- and LDS-limited),
// cached per (fn, lds). 1 when the query fails.
int resident_per_cu(const void* fn, int threads, size_t lds);

// Workgroups of 256 threads for a grid-stride walk over n elements: one thread per element, at least 1, at most cap.
inline int blocks_for(long long n, int cap) {
  long long b = (n + 255) / 256;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// The mixed-precision ladder: f(tag<TX>{}, tag<TY>{}) with TX / TY = float where xf / yf holds, bf16 elsewhere.
template <class T> struct tag { typedef T type; };
template <class Tag> using tag_t = typename Tag::type;
template <class F> int dispatch_xy(bool xf, bool yf, F&& f) {
  if (xf && yf) return f(tag<float>{}, tag<float>{});
  if (xf) return f(tag<float>{}, tag<bf16>{});
  if (yf) return f(tag<bf16>{}, tag<float>{});
  return f(tag<bf16>{}, tag<bf16>{});
}

}  // namespace vqa
