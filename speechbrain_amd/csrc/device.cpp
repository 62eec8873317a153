#include "device.h"

#include <atomic>
#include <map>
#include <mutex>
#include <utility>

namespace sbk {
namespace {
struct StreamWs {
  float* slabs;
  int* cnt;
};
std::mutex g_dev_mu;  // guards the two maps
std::map<std::pair<int, const void*>, size_t> g_lds_granted;  // (device, kernel) -> bytes
std::map<std::pair<int, hipStream_t>, StreamWs> g_stream_ws;
constexpr int kMaxDevices = 64;
std::atomic<int> g_cus[kMaxDevices];  // 0 = not asked yet

// two partial-tile slabs per workgroup: 512 workgroups x 128 x 128 (gemm.hip's kernels) or 256 x 256 x 256 (gemm_x3p.hip)
constexpr size_t kSkSlabBytes = (size_t)2 * 256 * 256 * 256 * sizeof(float);
static_assert(kSkSlabBytes >= (size_t)2 * kSkMaxGrid * 128 * 128 * sizeof(float), "slab area");
constexpr size_t kSkTicketBytes = (size_t)kSkMaxTiles * sizeof(int);
}  // namespace

int cur_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev;
}

int device_cus() {
  const int dev = cur_device();
  const bool cached = dev >= 0 && dev < kMaxDevices;
  int cus = cached ? g_cus[dev].load(std::memory_order_relaxed) : 0;
  if (cus) return cus;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (cus <= 0) cus = 256;
  if (cached) g_cus[dev].store(cus, std::memory_order_relaxed);  // (two first callers store the same value)
  return cus;
}

hipError_t allow_dyn_lds_fn(const void* kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;  // the window every kernel has
  const int dev = cur_device();
  std::lock_guard<std::mutex> lk(g_dev_mu);
  size_t& granted = g_lds_granted[std::make_pair(dev, kernel)];
  if (bytes <= granted) return hipSuccess;
  const hipError_t e = SBK_ALLOW_DYN_LDS(kernel, bytes);
  if (e == hipSuccess) granted = bytes;
  return e;
}

bool stream_ws(hipStream_t st, float** slabs, int** cnt) {
  const int dev = cur_device();
  std::lock_guard<std::mutex> lk(g_dev_mu);
  const auto it = g_stream_ws.find(std::make_pair(dev, st));
  if (it == g_stream_ws.end()) return false;
  *slabs = it->second.slabs;
  *cnt = it->second.cnt;
  return true;
}

int* tile_tickets(hipStream_t st, long tiles) {
  float* slabs;
  int* cnt;
  return tiles <= kSkMaxTiles && stream_ws(st, &slabs, &cnt) ? cnt : nullptr;
}
}  // namespace sbk

extern "C" size_t sbk_stream_workspace_bytes(void) { return sbk::kSkSlabBytes + sbk::kSkTicketBytes; }

extern "C" int sbk_stream_workspace_set(sbk_stream_t stream, void* workspace, size_t workspace_bytes) {
  SBK_REQUIRE(workspace && ((uintptr_t)workspace & 255) == 0, "stream workspace: null or not 256-byte aligned");
  SBK_REQUIRE(workspace_bytes >= sbk_stream_workspace_bytes(), "stream workspace: %zu bytes given, %zu needed", workspace_bytes,
              sbk_stream_workspace_bytes());
  hipStream_t st = sbk::as_stream(stream);
  sbk::StreamWs w{reinterpret_cast<float*>(workspace),
                  reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + sbk::kSkSlabBytes)};
  // tickets start at zero (ordered before the first launch on this stream); every launch leaves them at zero
  const hipError_t e = hipMemsetAsync(w.cnt, 0, sbk::kSkTicketBytes, st);
  if (e != hipSuccess) return sbk::fail((int)e, "stream workspace: memset: %s", hipGetErrorString(e));
  const int dev = sbk::cur_device();
  std::lock_guard<std::mutex> lk(sbk::g_dev_mu);
  sbk::g_stream_ws[std::make_pair(dev, st)] = w;
  return 0;
}

extern "C" int sbk_stream_workspace_release(sbk_stream_t stream) {
  const int dev = sbk::cur_device();
  std::lock_guard<std::mutex> lk(sbk::g_dev_mu);
  sbk::g_stream_ws.erase(std::make_pair(dev, sbk::as_stream(stream)));
  return 0;
}
