// sf_policy_memory.hpp — sf_policy_memory_rows: the recurrent state of many agents to and from rows of caller-owned device
// buffers in one stream-ordered launch (included by sf_policy.hip behind Policy and check_agents).  The network memory that
// goes with a forked arena (sf_snapshot_load): agent g's h[2][160] and action one-hot[9] are what Backbone keeps between
// calls (Modules.hpp:81), for a policy and for a reward model alike.
#pragma once

namespace sfp {

// One wavefront per agent, four per workgroup; lane l owns elements l, l + 64, l + 128 (< 160) of both h vectors, lanes
// 0..8 the one-hot.  The row index is read once per wavefront; -1 and everything outside [0, rows) ends the wavefront
// before an address is formed from it.  All seven loads are issued before the first store.
template <bool TO_ROWS>
__global__ __launch_bounds__(256) void k_memory_rows(float *h0, float *h1, float *action_input, float *d_h, float *d_action,
                                                     const int32_t *row_of_agent, int rows, int agents) {
  const int g = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  if (g >= agents) return;
  const int row = __builtin_amdgcn_readfirstlane(row_of_agent[g]);
  if ((unsigned)row >= (unsigned)rows) return;
  float *own[3] = {h0 + (size_t)g * HID, h1 + (size_t)g * HID, action_input + (size_t)g * ACT};
  float *out[3] = {d_h + (size_t)row * 2 * HID, d_h + (size_t)row * 2 * HID + HID, d_action + (size_t)row * ACT};
  float v[7];
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int e = lane + 64 * j;
      v[3 * k + j] = e < HID ? (TO_ROWS ? own[k] : out[k])[e] : 0.f;
    }
  v[6] = lane < ACT ? (TO_ROWS ? own[2] : out[2])[lane] : 0.f;
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int e = lane + 64 * j;
      if (e < HID) (TO_ROWS ? out[k] : own[k])[e] = v[3 * k + j];
    }
  if (lane < ACT) (TO_ROWS ? out[2] : own[2])[lane] = v[6];
}

// `bytes` bytes at q: device memory of the object's device, 4-byte aligned, wholly inside its allocation (the checks
// sf_policy_load_weights makes on its sources)
static int check_memory_rows_range(const Policy *p, const void *q, size_t bytes, const char *name) {
  const std::string n = std::string("sf_policy_memory_rows: ") + name;
  if (!q) return fail(SF_ERR_ARG, n + " is null");
  if (reinterpret_cast<uintptr_t>(q) & 3u) return fail(SF_ERR_ARG, n + " is not 4-byte aligned");
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, q) != hipSuccess || at.type != hipMemoryTypeDevice || at.device != p->device) {
    (void)hipGetLastError();  // (a host pointer is an error of the query: it is answered here, not left behind)
    return fail(SF_ERR_ARG, n + " is not device memory of the object's device");
  }
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(q)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(SF_ERR_ARG, n + ": its allocation is unknown to the runtime");
  }
  const uintptr_t lo = reinterpret_cast<uintptr_t>(base), addr = reinterpret_cast<uintptr_t>(q);
  if (addr < lo || addr - lo > size || bytes > size - (addr - lo)) return fail(SF_ERR_ARG, n + " reaches past the end of its allocation");
  return SF_OK;
}

static int memory_rows(Policy *p, int to_rows, float *d_h, float *d_action, const int32_t *d_row_of_agent, int rows, int agents) {
  SFP_RC(check_agents(p, agents));
  if (rows < 1) return fail(SF_ERR_ARG, "sf_policy_memory_rows: rows < 1");
  SFP_HIP(hipSetDevice(p->device));
  SFP_RC(check_memory_rows_range(p, d_h, (size_t)rows * 2 * HID * sizeof(float), "d_h"));
  SFP_RC(check_memory_rows_range(p, d_action, (size_t)rows * ACT * sizeof(float), "d_action"));
  SFP_RC(check_memory_rows_range(p, d_row_of_agent, (size_t)agents * sizeof(int32_t), "d_row_of_agent"));
  const dim3 grid((unsigned)((agents + 3) / 4));
  if (to_rows)
    hipLaunchKernelGGL(k_memory_rows<true>, grid, dim3(256), 0, p->stream, p->h[0], p->h[1], p->action_input, d_h, d_action, d_row_of_agent, rows, agents);
  else
    hipLaunchKernelGGL(k_memory_rows<false>, grid, dim3(256), 0, p->stream, p->h[0], p->h[1], p->action_input, d_h, d_action, d_row_of_agent, rows, agents);
  SFP_HIP(hipGetLastError());
  return SF_OK;
}

}  // namespace sfp
