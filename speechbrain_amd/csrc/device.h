// What the library knows per device and per stream (csrc/device.cpp): the CU count, the grid rules that follow from it, the
// dynamic-LDS windows already granted, and the caller-registered stream workspaces.  Host code only; safe from concurrent threads.
#pragma once
#include "common.h"

namespace sbk {

int cur_device();
int device_cus();  // CUs of the current device, queried once per device (256 when the query fails)

// Persistent grids: a multiple of 8 workgroups (one share on each of the 8 XCDs), at least 8.
static inline int xcd_grid(int want) { return want >= 8 ? (want / 8) * 8 : 8; }
// Whole-tile kernels (gemm_x3p.hip, gemm_lp256.hip): one workgroup per tile while every tile gets a CU of its own (*whole = 1),
// otherwise one workgroup per CU, rounded down to the XCDs, walking the tiles.
static inline int whole_tile_grid(int tiles, int cus, int* whole) {
  *whole = tiles <= cus;
  return *whole ? tiles : (cus / 8) * 8;
}

// Raise `kernel`'s dynamic-LDS window to `bytes` on the current device (gfx950: 160 KiB per CU, 64 KiB without asking).  The
// largest window granted per (device, kernel) is remembered: the driver is asked only for a larger one.
hipError_t allow_dyn_lds_fn(const void* kernel, size_t bytes);
template <class... A>
hipError_t allow_dyn_lds(void (*kernel)(A...), size_t bytes) {
  return allow_dyn_lds_fn(reinterpret_cast<const void*>(kernel), bytes);
}
// the same as a launcher's check: 0, or the driver's status with "<who>: cannot raise the LDS window to <bytes> B" recorded
template <class... A>
int require_dyn_lds(void (*kernel)(A...), size_t bytes, const char* who) {
  const hipError_t e = allow_dyn_lds(kernel, bytes);
  return e == hipSuccess ? 0 : fail((int)e, "%s: cannot raise the LDS window to %zu B", who, bytes);
}

// Stream workspaces are CALLER-OWNED device memory (sbk_stream_workspace_set, include/sbk.h): the library allocates
// nothing.  One per (device, stream): launches of one stream are ordered, so they can share the slabs and the tickets.
constexpr int kSkMaxGrid = 512, kSkMaxTiles = 1 << 16;  // workgroups / tiles of a launch that uses one
// the stream's partial-tile slabs and zeroed tile tickets; false when the caller has registered none for it
bool stream_ws(hipStream_t st, float** slabs, int** cnt);
int* tile_tickets(hipStream_t st, long tiles);  // the tickets alone (nullptr: no workspace registered for the stream, or too many tiles)

}  // namespace sbk
