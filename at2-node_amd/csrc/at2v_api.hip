// at2v_api.hip — the C ABI of include/at2v.h (host side): the one translation unit of the context code.
//
// A context owns, per device: a stream, the persistent-grid scratch for the per-lane A tables, and growable device
// buffers. Host batches are split by index range (aligned to 64 records = one wave chunk = two verdict words) across the
// context's devices; each shard runs upload -> verify -> download on its own streams, so shards overlap.
//
// The code is split by role into pieces that only this file includes, in dependency order (as at2v_kernels.hip does
// with at2v_kern_*.h). Helpers are in anonymous namespaces and the entry points get their C linkage from the
// declarations of include/at2v.h, so the library exports the C ABI and nothing else. This file keeps at2v_create,
// at2v_destroy, at2v_verify_batch_device, at2v_verify_transfers_device and at2v_get_info.
//   at2v_device_scope.h  DeviceScope: the caller's current device, restored on every return path (also at2v_host.hip)
//   at2v_stage_plan.h    HIP-free: chunk schedule, chunk layout, arena bytes, copy pieces of the host-buffer pipeline
//   at2v_api_ctx.h       DevBuf, Shard, HostCall, at2v_ctx, hip_code / AT2V_TRY, init_shard
//   at2v_api_bcomb.h     the process-wide registry of the combs of B
//   at2v_api_cache.h     SenderCache and its host protocol: claim slots, compaction, thrash guard, control words
//   at2v_api_launch.h    launch_shard: the one verify launch path (scratch sets, cached launches)
//   at2v_api_pipe.h      HostPipe: staging slots, SDMA uploads, issue_chunk / flush_chunk, a shard's chunks
//   at2v_api_hostcall.h  the host-buffer call slots; at2v_verify_batch, at2v_verify_batch_submit / _wait, and the same
//                        for transfers given by their fields: at2v_verify_transfers, at2v_verify_transfers_submit
//   at2v_api_hostmem.h   pinned host ranges; at2v_host_alloc / _free / _register / _unregister
//   at2v_api_sender.h    known senders; at2v_sender_preload / _unpin / _query
//   at2v_api_comm.h      RCCL; at2v_comm_*, at2v_verify_shard_gather_device, at2v_verify_batch_sharded
//   at2v_api_tools.h     record generator, signer, point decoding, reject reasons
#include <random>

#include "at2v_api_ctx.h"
#include "at2v_api_bcomb.h"
#include "at2v_api_cache.h"
#include "at2v_api_launch.h"
#include "at2v_api_pipe.h"
#include "at2v_api_hostcall.h"
#include "at2v_api_hostmem.h"
#include "at2v_api_sender.h"
#include "at2v_api_comm.h"
#include "at2v_api_tools.h"

int at2v_create(const at2v_opts* opts, at2v_ctx** out) {
  if (!out) return AT2V_E_INVALID;
  *out = nullptr;
  // a timing-experiment build (wrong verdicts) serves no context unless the process explicitly allows it
  if (library_experiments()) {
    const char* allow = std::getenv("AT2V_ALLOW_EXPERIMENT");
    if (!allow || std::strcmp(allow, "1") != 0) return AT2V_E_INVALID;
  }
  at2v_opts o{0, 1, AT2V_POLICY_DALEK_V1, 0, 0, 0, 0, 0};
  if (opts) o = *opts;
  if (o.num_gpus < 0 || o.num_gpus > 64) return AT2V_E_INVALID;
  if (o.policy != AT2V_POLICY_DALEK_V1 && o.policy != AT2V_POLICY_LIBSODIUM_1_0_18 &&
      o.policy != AT2V_POLICY_DALEK_V1_LEGACY && o.policy != AT2V_POLICY_ZIP215)
    return AT2V_E_INVALID;  // (3 is unassigned)
  if (o.flags & ~(AT2V_CTX_CPU_FALLBACK | AT2V_CTX_ADMIT_FIRST | AT2V_CTX_BCOMB_WIDE)) return AT2V_E_INVALID;
  if (o.num_gpus == 0) {  // the CPU batch backend: no HIP call at all
    at2v_ctx* c = new (std::nothrow) at2v_ctx;
    if (!c) return AT2V_E_OOM;
    c->policy = o.policy;
    c->flags = o.flags;
    c->cpu = at2v::cpu_pool_create(o.cpu_threads);
    if (!c->cpu) {
      delete c;
      return AT2V_E_OOM;
    }
    *out = c;
    return AT2V_OK;
  }
  // AT2V_TEST_DEVICE_ALIAS (tests only): shard g runs on device (device + g) % ndev, so a one-GPU box executes the
  // single-process multi-device path (split, per-shard streams, scratch, B tables and caches) with num_gpus > ndev
  const bool alias = at2v::test_env_long("AT2V_TEST_DEVICE_ALIAS", 0) != 0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return AT2V_E_NODEVICE;
  if (o.device < 0 || o.device >= ndev || (!alias && o.device + o.num_gpus > ndev)) return AT2V_E_NODEVICE;
  at2v_ctx* c = new (std::nothrow) at2v_ctx;
  if (!c) return AT2V_E_OOM;
  c->policy = o.policy;
  c->flags = o.flags;
  c->test_fail_launches = (uint32_t)at2v::test_env_long("AT2V_TEST_FAIL_LAUNCH", 0);
  c->partition = at2v::test_env_long("AT2V_CACHE_PARTITION", 1) != 0;  // (A/B: 0 = round 4)
  c->stage_first = (size_t)at2v::test_env_long("AT2V_TEST_STAGE_FIRST", (long)at2v::kStageFirstRecords) / 64 * 64;
  c->stage_max = (size_t)at2v::test_env_long("AT2V_TEST_STAGE_MAX", (long)at2v::kStageMaxRecords) / 64 * 64;
  c->copy_threads = (unsigned)at2v::test_env_long("AT2V_TEST_COPY_THREADS", 8);
  c->pipe_streams = (int)at2v::test_env_long("AT2V_TEST_PIPE_STREAMS", c->pipe_streams);
  c->pipe_trace = at2v::test_env_long("AT2V_TEST_PIPE_TRACE", 0) != 0;
  if (c->stage_first < 64) c->stage_first = 64;
  if (c->stage_max < c->stage_first) c->stage_max = c->stage_first;
  c->pair_max = o.small_batch_max == 0 ? AT2V_SMALL_BATCH_DEFAULT
                : o.small_batch_max == AT2V_SMALL_BATCH_OFF ? 0u : o.small_batch_max;
  c->shards.resize((size_t)o.num_gpus);
  const DeviceScope keep;
  std::random_device rd;
  // test hook (A/B runs of processes the caller does not configure, e.g. the config-5 mini-network's nodes)
  const bool wide_env = at2v::test_env_long("AT2V_BCOMB_WIDE", 0) != 0;
  for (int g = 0; g < o.num_gpus; ++g) {
    int rc = init_shard(c->shards[(size_t)g], alias ? (o.device + g) % ndev : o.device + g);
    if (rc == AT2V_OK && o.sender_cache)
      rc = init_cache(c->shards[(size_t)g], o.sender_cache, ((uint64_t)rd() << 32) ^ rd(), o.sender_comb != 0,
                      (o.flags & AT2V_CTX_ADMIT_FIRST) != 0, (o.flags & AT2V_CTX_BCOMB_WIDE) != 0 || wide_env);
    // the cross-rank failure flag of at2v_comm_init_rank / at2v_verify_batch_sharded (first device): allocated here,
    // so a rank whose communicator set-up fails can still join the outcome all-reduce
    if (rc == AT2V_OK && g == 0) rc = hip_code(c->status.ensure(4));
    if (rc == AT2V_OK && g == 0 && (o.flags & AT2V_CTX_CPU_FALLBACK)) {
      c->cpu = at2v::cpu_pool_create(o.cpu_threads);
      if (!c->cpu) rc = AT2V_E_OOM;
    }
    if (rc != AT2V_OK) {
      at2v_destroy(c);
      return rc;
    }
  }
  *out = c;
  return AT2V_OK;
}

void at2v_destroy(at2v_ctx* ctx) {
  if (!ctx) return;
  // drain first: the last all-gather may still run on a caller's stream, and verify launches on the
  // shard streams or on callers' streams are ordered before each shard's scratch_free event
  for (Shard& s : ctx->shards) {
    if (hipSetDevice(s.device) != hipSuccess) continue;
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.pipe) sync_pipe_streams(*s.pipe);
    for (hipEvent_t ev : s.scratch_free)
      if (ev) (void)hipEventSynchronize(ev);
  }
  if (ctx->comm) {
    (void)hipSetDevice(ctx->shards.empty() ? 0 : ctx->shards[0].device);
    if (ctx->gather_done) (void)hipEventSynchronize(ctx->gather_done);
    (void)ncclCommFinalize(ctx->comm);
    (void)ncclCommDestroy(ctx->comm);
    ctx->comm = nullptr;
  }
  if (ctx->gather_done) (void)hipEventDestroy(ctx->gather_done);
  for (DevBuf* b : {&ctx->window, &ctx->zeros, &ctx->zeros_big, &ctx->status}) b->release();
  for (Shard& s : ctx->shards) {
    if (hipSetDevice(s.device) != hipSuccess) continue;
    for (hipEvent_t ev : s.scratch_free)
      if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : s.hcopied)
      if (ev) (void)hipEventDestroy(ev);
    for (DevBuf& b : s.hverdict) b.release();
    for (DevBuf& b : s.hrok) b.release();
    free_pipe(s);
    free_cache(s.cache);
    for (DevBuf& b : s.scratch) b.release();
    for (DevBuf& b : s.part) b.release();
    for (DevBuf* b : {&s.btab, &s.pk, &s.sig, &s.verdict, &s.reasons}) b->release();
    if (s.stream) (void)hipStreamDestroy(s.stream);
  }
  // the pinned host ranges still known (every upload from them has landed: free_pipe waited for the slots' signals)
  for (const at2v::HostRange& r : ctx->hostmem.ranges())
    (void)release_host_range(ctx, reinterpret_cast<void*>(r.base), r.owned);
  at2v::cpu_pool_destroy(ctx->cpu);
  at2v::cpu_pool_destroy(ctx->copier);
  delete ctx;
}

int at2v_verify_batch_device(at2v_ctx* ctx, const uint8_t* d_pk, const uint8_t* d_sig, const uint8_t* d_msg,
                             size_t msg_bytes, const uint32_t* d_msg_off, size_t n, uint32_t* d_verdicts,
                             void* hip_stream) {
  if (!ctx) return AT2V_E_INVALID;
  if (n == 0) return AT2V_OK;
  if (!d_pk || !d_sig || !d_msg_off || !d_verdicts || n >= (1u << 31) || msg_bytes >= (1ull << 32))
    return AT2V_E_INVALID;
  if (ctx->shards.empty()) return AT2V_E_NODEVICE;
  if (!aligned(d_pk, 16) || !aligned(d_sig, 16) || !aligned(d_msg_off, 4) || !aligned(d_verdicts, 4))
    return AT2V_E_ALIGN;
  Shard& s = ctx->shards[0];
  const DeviceScope scope(s.device);
  hipError_t e = scope.err;
  if (e == hipSuccess)
    e = launch_shard(ctx, s, d_pk, d_sig, d_msg, (uint32_t)msg_bytes, d_msg_off, (uint32_t)n, d_verdicts,
                     (hipStream_t)hip_stream);
  return hip_code(e);
}

// The workspace of the device form: offsets (n + 1) | messages (n x L) | the kernels' 16 bytes of slack, both parts
// 16-byte aligned.
size_t at2v_transfers_workspace_bytes(size_t n, int wire) {
  const size_t len = at2v::transfer_msg_len(wire);
  if (len == 0 || n >= (1u << 31) || (uint64_t)n * len >= (1ull << 32)) return 0;
  return (((n + 1) * 4 + 15) & ~(size_t)15) + n * len + 16;
}

int at2v_verify_transfers_device(at2v_ctx* ctx, const uint8_t* d_sender, const uint8_t* d_sig,
                                 const uint8_t* d_recipient, const uint64_t* d_amount, size_t n, int wire, void* d_work,
                                 size_t work_bytes, uint32_t* d_verdicts, uint32_t* d_recipient_ok, void* hip_stream) {
  if (!ctx) return AT2V_E_INVALID;
  const size_t len = at2v::transfer_msg_len(wire);
  if (len == 0) return AT2V_E_INVALID;
  if (n == 0) return AT2V_OK;
  const size_t need = at2v_transfers_workspace_bytes(n, wire);  // (0: an n the generated uint32 offsets cannot serve)
  if (!d_sender || !d_sig || !d_recipient || !d_amount || !d_work || !d_verdicts || need == 0 || work_bytes < need)
    return AT2V_E_INVALID;
  if (ctx->shards.empty()) return AT2V_E_NODEVICE;
  if (!aligned(d_sender, 16) || !aligned(d_sig, 16) || !aligned(d_recipient, 16) || !aligned(d_amount, 8) ||
      !aligned(d_work, 16) || !aligned(d_verdicts, 4) || (d_recipient_ok && !aligned(d_recipient_ok, 4)))
    return AT2V_E_ALIGN;
  Shard& s = ctx->shards[0];
  const DeviceScope scope(s.device);
  uint32_t* d_off = static_cast<uint32_t*>(d_work);
  uint8_t* d_msg = static_cast<uint8_t*>(d_work) + (((n + 1) * 4 + 15) & ~(size_t)15);
  hipError_t e = scope.err;
  if (e == hipSuccess)
    e = at2v::launch_transfer_prep(d_recipient, d_amount, (uint32_t)n, wire, d_msg, d_off, d_recipient_ok,
                                   (hipStream_t)hip_stream);
  if (e == hipSuccess)
    e = launch_shard(ctx, s, d_sender, d_sig, d_msg, (uint32_t)(n * len), d_off, (uint32_t)n, d_verdicts,
                     (hipStream_t)hip_stream);
  return hip_code(e);
}

const char* at2v_strerror(int code) {
  switch (code) {
    case AT2V_OK: return "ok";
    case AT2V_E_INVALID: return "invalid argument";
    case AT2V_E_NODEVICE: return "no usable gfx950 device (or a device entry point on a CPU context)";
    case AT2V_E_HIP: return "HIP runtime error";
    case AT2V_E_OOM: return "out of memory";
    case AT2V_E_ALIGN: return "misaligned device pointer";
    case AT2V_E_RCCL: return "RCCL error";
    case AT2V_E_PEER: return "another rank failed this collective batch (its records are verdict 0)";
    default: return "unknown error";
  }
}

int at2v_get_info(at2v_ctx* ctx, at2v_info* out) {
  if (!ctx || !out) return AT2V_E_INVALID;
  std::memset(out, 0, sizeof *out);
  out->cpu_threads = at2v::cpu_pool_threads(ctx->cpu);
  out->cpu_batches = ctx->cpu_batches;
  out->cpu_fallbacks = ctx->cpu_fallbacks;
  out->experiments = library_experiments();
  out->host_chunks = ctx->host_chunks;
  out->host_direct_bytes = ctx->host_direct_bytes;
  out->host_staged_bytes = ctx->host_staged_bytes;
  if (ctx->shards.empty()) return AT2V_OK;  // CPU context: no device geometry
  const Shard& s = ctx->shards[0];
  out->num_gpus = (int)ctx->shards.size();
  out->grid_blocks = s.grid;
  out->block_threads = at2v::block_threads();
  out->waves_per_cu = s.blocks_per_cu * at2v::block_threads() / 64;
  out->cus = s.cus;
  out->vgprs = s.vgprs;
  out->rank = ctx->rank;
  out->world = ctx->comm ? ctx->world : 0;
  out->gathers = ctx->gathers;
  for (const Shard& sh : ctx->shards) {
    // sender-cache counters, summed over devices. Waits for the context's cache work only (its build stream, which
    // follows every cached launch): builds of earlier launches are done and their keys usable when this returns.
    if (!sh.cache) continue;
    CtlWords w;
    const DeviceScope scope(sh.device);
    if (scope.err != hipSuccess || hipStreamSynchronize(sh.cache->build) != hipSuccess ||
        read_ctl(*sh.cache, w, /*wait=*/true) != hipSuccess)
      continue;
    const uint64_t cap = sh.cache->args.capacity;
    out->cache_entries += cap - payloads_free(w, cap);  // keys holding a payload
    out->cache_chunks += w[at2v::kCtlChunks];
    out->cache_chunk_hits += w[at2v::kCtlChunkHits];
    out->cache_claims += w[at2v::kCtlClaimed];
    out->cache_evicted += w[at2v::kCtlEvicted];
    out->cache_compactions += w[at2v::kCtlCompactions];
    out->cache_sightings += w[at2v::kCtlSighted];
    out->cache_built += w[at2v::kCtlBuilt];
    out->cache_record_hits += w[at2v::kCtlRecHits];
    int khz = 0;  // device wall clock (wall_clock64) in kHz
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, sh.device) == hipSuccess && khz > 0)
      out->cache_build_us += w[at2v::kCtlBuildTicks] * 1000ull / (uint64_t)khz;
    out->cache_capacity += cap;
  }
  return AT2V_OK;
}

int at2v_abi_version(void) { return AT2V_ABI_VERSION; }
