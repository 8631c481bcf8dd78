// at2v_api_hostmem.h — pinned host memory: at2v_host_alloc / _free / _register / _unregister (part of the one
// translation unit at2v_api.hip; the registry itself is at2v_hostmem.h).
// A CPU context only records the ranges: every hip* / hsa* call below is behind `ctx->shards.empty()`.
#pragma once
#include "at2v_api_hostcall.h"

namespace {

void* pointer_info_alloc(size_t bytes) { return std::malloc(bytes); }

bool hsa_ready(at2v_ctx* ctx) {  // (HIP already initialised the runtime; hsa_init only takes a reference, as in ensure_pipe)
  if (!ctx->hsa_ref) ctx->hsa_ref = hsa_init() == HSA_STATUS_SUCCESS;
  return ctx->hsa_ref;
}

// the device agents of the context's shards, each once (aliased shards share one): the owners of their B tables
bool shard_agents(at2v_ctx* ctx, std::vector<hsa_agent_t>& out) {
  for (const Shard& s : ctx->shards) {
    hsa_amd_pointer_info_t di;
    std::memset(&di, 0, sizeof di);
    di.size = sizeof di;
    if (hsa_amd_pointer_info(s.btab.p, &di, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS || !di.agentOwner.handle)
      return false;
    bool seen = false;
    for (const hsa_agent_t& a : out) seen = seen || a.handle == di.agentOwner.handle;
    if (!seen) out.push_back(di.agentOwner);
  }
  return !out.empty();
}

// What the runtime says about the pinned range [p, p + bytes) of a GPU context: AT2V_OK and the address the DMA engine
// is given for p (the range's agent address; for memory pinned in place it differs from the host address), or
// AT2V_E_INVALID unless the runtime reports the whole range as one pinned allocation (its own, or locked in place)
// that every shard's device can reach. A copy from an address a device cannot read is a GPU fault, not an error code:
// this check keeps such a copy from ever being submitted.
// `locked`: what hsa_amd_memory_lock returned for p (at2v_host_register), nullptr for the runtime's own allocation. On
// an MI355X the runtime maps memory locked in place into the devices at its own address (shared virtual memory) and
// hsa_amd_pointer_info does not know such a range (type unknown; memory pinned by hipHostRegister reads the same). The
// runtime's report is then its access query: every device must have access to every page of the range.
int pinned_range_dma(at2v_ctx* ctx, const void* p, size_t bytes, const void* locked, uintptr_t* dma) {
  if (!hsa_ready(ctx)) return AT2V_E_HIP;
  std::vector<hsa_agent_t> gpus;
  if (!shard_agents(ctx, gpus)) return AT2V_E_HIP;
  hsa_amd_pointer_info_t info;
  std::memset(&info, 0, sizeof info);
  info.size = sizeof info;
  uint32_t na = 0;
  hsa_agent_t* acc = nullptr;
  if (hsa_amd_pointer_info(p, &info, pointer_info_alloc, &na, &acc) != HSA_STATUS_SUCCESS) return AT2V_E_INVALID;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p), hb = reinterpret_cast<uintptr_t>(info.hostBaseAddress);
  if (info.type == HSA_EXT_POINTER_TYPE_UNKNOWN && locked == p) {
    std::free(acc);
    const uintptr_t page = 4096, lo = a & ~(page - 1), hi = (a + bytes + page - 1) & ~(page - 1);
    for (const hsa_agent_t& g : gpus) {
      hsa_amd_svm_attribute_pair_t q{HSA_AMD_SVM_ATTRIB_ACCESS_QUERY, g.handle};
      if (hsa_amd_svm_attributes_get(reinterpret_cast<void*>(lo), hi - lo, &q, 1) != HSA_STATUS_SUCCESS) return AT2V_E_INVALID;
      if (q.attribute != HSA_AMD_SVM_ATTRIB_AGENT_ACCESSIBLE && q.attribute != HSA_AMD_SVM_ATTRIB_AGENT_ACCESSIBLE_IN_PLACE)
        return AT2V_E_INVALID;
    }
    *dma = a;
    return AT2V_OK;
  }
  bool ok = (info.type == HSA_EXT_POINTER_TYPE_HSA || info.type == HSA_EXT_POINTER_TYPE_LOCKED) &&
            info.agentBaseAddress && info.hostBaseAddress && hb <= a && a + bytes <= hb + info.sizeInBytes;
  for (size_t g = 0; g < gpus.size() && ok; ++g) {
    bool reach = false;
    for (uint32_t i = 0; i < na; ++i) reach = reach || acc[i].handle == gpus[g].handle;
    ok = reach;
  }
  std::free(acc);
  if (!ok) return AT2V_E_INVALID;
  *dma = reinterpret_cast<uintptr_t>(info.agentBaseAddress) + (a - hb);
  if (locked && *dma != reinterpret_cast<uintptr_t>(locked)) return AT2V_E_INVALID;  // (the lock and the report disagree)
  return AT2V_OK;
}

// gives a range's memory back: an allocation (`owned`) is freed, a registered range unlocked; a CPU context only frees
int release_host_range(const at2v_ctx* ctx, void* p, bool owned) {
  if (ctx->shards.empty()) {
    if (owned) std::free(p);
    return AT2V_OK;
  }
  if (owned) return hip_code(hipHostFree(p));
  return hsa_amd_memory_unlock(p) == HSA_STATUS_SUCCESS ? AT2V_OK : AT2V_E_HIP;
}

// at2v_host_free (`owned`) / at2v_host_unregister: p starts a known range of that kind; no call in flight reads it
int forget_host_range(at2v_ctx* ctx, void* p, bool owned) {
  if (!ctx || !p) return AT2V_E_INVALID;
  const at2v::HostRange* r = ctx->hostmem.at(p);
  if (!r || r->owned != owned) return AT2V_E_INVALID;
  quiesce_host_calls(ctx);
  ctx->hostmem.remove(p);
  return release_host_range(ctx, p, owned);
}

}  // namespace

int at2v_host_alloc(at2v_ctx* ctx, size_t bytes, void** out) {
  if (!ctx || !out) return AT2V_E_INVALID;
  *out = nullptr;
  if (bytes == 0 || bytes > (~(size_t)0 >> 1)) return AT2V_E_INVALID;
  at2v::HostRange r;
  r.len = bytes;
  r.owned = true;
  const bool cpu = ctx->shards.empty();  // CPU context: plain host memory, no device is touched
  void* p = nullptr;
  // portable: pinned for and mapped to every device, whichever is current (page-aligned, so 64-byte aligned)
  if (cpu) p = std::aligned_alloc(64, (bytes + 63) & ~(size_t)63);
  else if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) p = nullptr;
  if (!p) return AT2V_E_OOM;
  r.base = reinterpret_cast<uintptr_t>(p);
  int rc = cpu ? AT2V_OK : pinned_range_dma(ctx, p, bytes, nullptr, &r.dma);
  if (rc == AT2V_OK && !ctx->hostmem.insert(r)) rc = AT2V_E_INVALID;
  if (rc == AT2V_OK) *out = p;
  else (void)release_host_range(ctx, p, true);
  return rc;
}

int at2v_host_free(at2v_ctx* ctx, void* p) { return forget_host_range(ctx, p, true); }

int at2v_host_register(at2v_ctx* ctx, void* p, size_t bytes) {
  if (!ctx || !p || bytes == 0) return AT2V_E_INVALID;
  at2v::HostRange r;
  r.base = reinterpret_cast<uintptr_t>(p);
  r.len = bytes;
  if (r.base + bytes < r.base) return AT2V_E_INVALID;
  if (ctx->shards.empty()) return ctx->hostmem.insert(r) ? AT2V_OK : AT2V_E_INVALID;  // CPU context: recorded only
  // an overlap with a known range is refused before the runtime is asked to pin anything
  if (!ctx->hostmem.insertable(r.base, r.len)) return AT2V_E_INVALID;
  // Locked through the HSA runtime for exactly the devices of the context (what hipHostRegister does underneath, for
  // every device). The lock returns the address the devices see the range at; the runtime's own report of the range
  // must confirm it (pinned_range_dma), or the registration is refused.
  std::vector<hsa_agent_t> gpus;
  if (!hsa_ready(ctx) || !shard_agents(ctx, gpus)) return AT2V_E_HIP;
  void* agent_ptr = nullptr;
  if (hsa_amd_memory_lock(p, bytes, gpus.data(), (int)gpus.size(), &agent_ptr) != HSA_STATUS_SUCCESS || !agent_ptr)
    return AT2V_E_OOM;
  int rc = pinned_range_dma(ctx, p, bytes, agent_ptr, &r.dma);
  if (rc == AT2V_OK && !ctx->hostmem.insert(r)) rc = AT2V_E_INVALID;
  if (rc != AT2V_OK) (void)hsa_amd_memory_unlock(p);
  return rc;
}

int at2v_host_unregister(at2v_ctx* ctx, void* p) { return forget_host_range(ctx, p, false); }
