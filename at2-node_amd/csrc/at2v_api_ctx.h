// at2v_api_ctx.h — the context and its per-device shards (a piece of at2v_api.hip, as every at2v_api_*.h).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <set>
#include <vector>

#include "../../include/at2v.h"
#include "at2v_cpu.h"
#include "at2v_device_scope.h"
#include "at2v_env.h"
#include "at2v_hostmem.h"
#include "at2v_launch.h"
#include "at2v_stage_plan.h"
#include "at2v_transfer.h"

namespace {

using at2v::DeviceScope;

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 4, 4096);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

// scratch sets per device (AT2V_SCRATCH_SETS overrides, 1..4; 1 = every launch waits for the previous one)
constexpr int kScratchSets = 2;

struct SenderCache;  // at2v_api_cache.h
struct HostPipe;     // at2v_api_pipe.h

struct Shard {
  int device = 0;
  hipStream_t stream = nullptr;
  int sets = kScratchSets;
  unsigned next_set = 0;
  hipEvent_t scratch_free[4] = {};  // per set: recorded after the launch that last used it; the set's next launch waits
  int grid = 0;  // persistent grid (blocks)
  int cus = 0;
  int blocks_per_cu = 0;
  int vgprs = 0;
  DevBuf scratch[4];
  DevBuf part[4];  // per scratch set: the classify kernel's hit / miss lists (partitioned cached launches)
  DevBuf btab, pk, sig, verdict;
  DevBuf reasons;                // at2v_reject_reasons (host buffers): the gathered rejects' reason bytes
  DevBuf hverdict[3];            // host-buffer calls: the shard's device bitmap per call slot (HostCall)
  hipEvent_t hcopied[3] = {nullptr, nullptr, nullptr};  // ... and its verdict copy (the call waits for this, not for
                                                        // the cache builds behind it)
  DevBuf hrok[3];                // transfers calls that ask for recipient_ok: that bitmap, beside hverdict
  SenderCache* cache = nullptr;
  HostPipe* pipe = nullptr;     // the host-buffer path's streams and staging (created by the first host-buffer call)
};

}  // namespace

// A host-buffer call in flight. Slots 0 and 1: at2v_verify_batch_submit (slot = ticket % 2; at most two in flight, each
// with its own device bitmap and arena per shard, so the host stages the second while the first one's launches run and
// the device sees no gap between them). Slot 2: the synchronous at2v_verify_batch, after the calls in flight are
// complete (their results stay for their waits).
struct HostBatch {  // the caller's arrays of a host-buffer call (at2v_verify_batch's arguments)
  const uint8_t *pk = nullptr, *sig = nullptr, *msg = nullptr;
  const uint32_t* msg_off = nullptr;
  size_t n = 0;
  uint32_t* verdicts = nullptr;
  // a transfers call (at2v_verify_transfers*): pk holds the senders, msg and msg_off are null, and the messages are
  // built from these fields (at2v_transfer.h) on the device, or on the CPU backend's stack
  bool transfers = false;
  const uint8_t* recipient = nullptr;
  const uint64_t* amount = nullptr;
  int wire = 0;
  uint32_t* recipient_ok = nullptr;  // ceil(n / 32) words out, or null
  // message bytes of records [lo, hi)
  size_t msg_bytes(size_t lo, size_t hi) const {
    return transfers ? (hi - lo) * at2v::transfer_msg_len(wire) : (size_t)(msg_off[hi] - msg_off[lo]);
  }
};
struct HostCall {
  bool active = false, done = false;
  uint64_t ticket = 0;
  int rc = 0;
  HostBatch b;
  std::vector<hipError_t> err;  // per shard
  std::vector<size_t> m;        // per shard: records
  std::chrono::steady_clock::time_point t0;
};

struct at2v_ctx {
  at2v_policy policy = AT2V_POLICY_DALEK_V1;
  uint32_t pair_max = AT2V_SMALL_BATCH_DEFAULT;  // launches of <= this many records: low-latency kernel
  uint32_t flags = 0;         // at2v_opts.flags (AT2V_CTX_*)
  std::vector<Shard> shards;  // empty: a CPU-backend context (at2v_opts.num_gpus = 0)
  at2v::CpuPool* cpu = nullptr;  // the CPU backend (a CPU context, or AT2V_CTX_CPU_FALLBACK)
  at2v::CpuPool* copier = nullptr;  // the host-buffer path's staging copies (created by the first host-buffer call)
  // atomic: an ingest queue with AT2V_QUEUE_CPU_FALLBACK may fall back from its launcher and its completer thread at once
  // (both call at2v_verify_batch on the queue's CPU context; the pool serialises the work itself)
  std::atomic<uint64_t> cpu_batches{0}, cpu_fallbacks{0};
  // the host-buffer path's chunk schedule (HostPipe; test hooks AT2V_TEST_STAGE_FIRST / _MAX / AT2V_TEST_COPY_THREADS)
  size_t stage_first = at2v::kStageFirstRecords, stage_max = at2v::kStageMaxRecords;
  unsigned copy_threads = 8;
  int pipe_streams = 0;     // create_comp_stream mode (test hook AT2V_TEST_PIPE_STREAMS)
  bool pipe_trace = false;  // test hook AT2V_TEST_PIPE_TRACE: per host-buffer call, where the host's time went (stderr)
  double tr_wait = 0, tr_copy = 0, tr_enq = 0;  // seconds, this call
  uint64_t host_chunks = 0;  // chunks staged by host-buffer calls (at2v_info.host_chunks)
  // pinned host ranges handed over through at2v_host_alloc / at2v_host_register: a slice of pk, sig or msg that lies
  // wholly inside one of them is uploaded from the caller's memory, without the copy into a staging slot (issue_chunk)
  at2v::HostRegistry hostmem;
  uint64_t host_direct_bytes = 0, host_staged_bytes = 0;  // at2v_info: pk/sig/msg bytes uploaded either way
  bool hsa_ref = false;  // at2v_host_alloc / _register took their reference on the HSA runtime (hsa_init)
  uint32_t test_fail_launches = 0;  // AT2V_TEST_FAIL_LAUNCH (tests only): that many launches fail before the kernel
  bool partition = true;  // cached launches above pair_max classify, then verify hits and misses apart (AT2V_CACHE_PARTITION)
  ncclComm_t comm = nullptr;  // at2v_comm_init_rank (one rank per process, the context's first device)
  int rank = 0, world = 1;
  DevBuf window;              // at2v_verify_batch_sharded: world x kGatherWindow words, one all-gather round
  DevBuf zeros;               // >= kGatherWindow zero words: what a rank that failed locally sends
  DevBuf zeros_big;           // zero words for at2v_verify_shard_gather_device calls with words_per_rank > kGatherWindow
  DevBuf status;              // one int32: the cross-rank failure flag (agree_on_failure)
  hipEvent_t gather_done = nullptr;  // recorded after every all-gather, on its stream (at2v_destroy waits for it)
  uint64_t gathers = 0;       // all-gathers issued (at2v_info.gathers)
  HostCall calls[3];          // host-buffer call slots (HostCall)
  // at2v_sender_preload with AT2V_SENDER_PIN: the pinned keys, deduplicated here, so the capacity / 2 limit is exact and
  // costs no device work (the entries' pin marks on the devices follow this set)
  std::set<std::array<uint8_t, 32>> pinned;
  uint64_t next_ticket = 1;
};

namespace {

int hip_code(hipError_t e) {
  if (e == hipSuccess) return AT2V_OK;
  if (e == hipErrorOutOfMemory) return AT2V_E_OOM;
  if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorNoBinaryForGpu) return AT2V_E_NODEVICE;
  return AT2V_E_HIP;
}

#define AT2V_TRY(expr)                       \
  do {                                       \
    hipError_t e_ = (expr);                  \
    if (e_ != hipSuccess) return hip_code(e_); \
  } while (0)

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// AT2V_EXPERIMENT_* bits of this library (the kernels object has no experiment builds any more)
unsigned library_experiments() {
  unsigned m = 0;
#if AT2V_EXP_BCOMB_NOBUILD
  m |= AT2V_EXPERIMENT_BCOMB_NOBUILD;
#endif
  return m;
}

int init_shard(Shard& s, int device) {
  s.device = device;
  AT2V_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  AT2V_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return AT2V_E_NODEVICE;
  s.cus = prop.multiProcessorCount;
  AT2V_TRY(at2v::verify_occupancy(&s.blocks_per_cu, &s.vgprs));
  if (s.blocks_per_cu < 1) s.blocks_per_cu = 1;
  s.grid = s.cus * s.blocks_per_cu;
  AT2V_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
  for (hipEvent_t& ev : s.hcopied) AT2V_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));  // (3 slots)
  if (const char* v = at2v::test_env("AT2V_SCRATCH_SETS")) s.sets = std::min(4, std::max(1, std::atoi(v)));
  for (int j = 0; j < s.sets; ++j) {
    AT2V_TRY(hipEventCreateWithFlags(&s.scratch_free[j], hipEventDisableTiming));
    AT2V_TRY(hipEventRecord(s.scratch_free[j], s.stream));
    AT2V_TRY(s.scratch[j].ensure(at2v::scratch_bytes(s.grid)));
  }
  // fixed-base tables [0..2^15]B and [0..2^15] 2^128 B, built on the device once per context
  AT2V_TRY(s.btab.ensure(at2v::btab_bytes()));
  AT2V_TRY(at2v::launch_build_btab((int4*)s.btab.p, s.stream));
  AT2V_TRY(hipStreamSynchronize(s.stream));
  return AT2V_OK;
}

}  // namespace
