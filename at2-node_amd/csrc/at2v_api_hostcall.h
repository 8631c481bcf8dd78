// at2v_api_hostcall.h — the host-buffer calls and their slots: at2v_verify_batch, at2v_verify_batch_submit / _wait, and
// at2v_verify_transfers / _submit, which take the fields of AT2 transfers instead of messages (a piece of at2v_api.hip).
// A call's records go through every shard's pipe (at2v_api_pipe.h).
#pragma once
#include <cstdio>

#include "at2v_api_pipe.h"
#include "at2v_shard.h"

namespace {

// Issue a host-buffer call into slot k: per shard (64-aligned index range: its words start at word lo/32 of the caller's
// array) the device bitmap and the pipe, then the chunks of all shards round robin, so every device's pipeline fills
// early and the copy pool serves them in turn; then the verdict copies. Returns once everything is enqueued (the host
// copies are done; the launches and downloads run on).
void host_call_issue(at2v_ctx* ctx, int k) {
  HostCall& hc = ctx->calls[k];
  const HostBatch& b = hc.b;
  const size_t G = ctx->shards.size();
  at2v::CpuPool* copier = copy_pool(ctx);
  std::vector<ChunkPlan> plan(G);
  std::vector<size_t> lo(G);
  std::vector<hipError_t>& err = hc.err;
  err.assign(G, hipSuccess);
  hc.m.assign(G, 0);
  hc.t0 = std::chrono::steady_clock::now();
  ctx->tr_wait = ctx->tr_copy = ctx->tr_enq = 0;
  for (size_t g = 0; g < G; ++g) {
    Shard& s = ctx->shards[g];
    const at2v::Range r = at2v::device_range(b.n, G, g);
    lo[g] = r.lo;
    plan[g].init(r.size(), ctx->pair_max, ctx->stage_first, ctx->stage_max);
    hc.m[g] = r.size();
    if (r.size() == 0) continue;
    hipError_t e = hipSetDevice(s.device);
    if (e == hipSuccess) e = s.hverdict[k].ensure(((r.size() + 31) / 32) * 4);
    if (e == hipSuccess && b.recipient_ok) e = s.hrok[k].ensure(((r.size() + 31) / 32) * 4);
    if (e == hipSuccess) e = ensure_pipe(s, ctx->pipe_streams);
    if (e == hipSuccess) s.pipe->cur = k;
    if (e == hipSuccess) e = begin_arena(ctx, s, r.size(), b.msg_bytes(r.lo, r.hi), b.transfers);
    err[g] = e;
  }
  for (bool more = true; more;) {
    more = false;
    for (size_t g = 0; g < G; ++g) {
      if (err[g] != hipSuccess || plan[g].done()) continue;
      Shard& s = ctx->shards[g];
      err[g] = hipSetDevice(s.device);
      if (err[g] == hipSuccess)
        err[g] = issue_next_chunk(ctx, s, copier, b, plan[g], lo[g], (uint32_t*)s.hverdict[k].p,
                                  b.recipient_ok ? (uint32_t*)s.hrok[k].p : nullptr);
      more = more || !plan[g].done();
    }
  }
  for (size_t g = 0; g < G; ++g) {  // the last chunk of every shard
    Shard& s = ctx->shards[g];
    if (hc.m[g] == 0 || !s.pipe) continue;
    hipError_t e = hipSetDevice(s.device);
    if (e == hipSuccess) e = flush_chunk(ctx, s);
    if (err[g] == hipSuccess) err[g] = e;
  }
  // the verdict words of each shard (and a transfers call's recipient_ok words: same word offsets, same stream, same
  // event), once its last two launches are done (copy stream)
  for (size_t g = 0; g < G; ++g) {
    Shard& s = ctx->shards[g];
    const size_t m = hc.m[g];
    if (m == 0) continue;
    hipError_t e = err[g];
    if (e == hipSuccess) e = hipSetDevice(s.device);
    HostPipe* p = s.pipe;
    if (e == hipSuccess) e = wait_for_chunks(*p, p->copy);
    if (e == hipSuccess)
      e = hipMemcpyAsync(b.verdicts + lo[g] / 32, s.hverdict[k].p, ((m + 31) / 32) * 4, hipMemcpyDeviceToHost, p->copy);
    if (e == hipSuccess && b.recipient_ok)
      e = hipMemcpyAsync(b.recipient_ok + lo[g] / 32, s.hrok[k].p, ((m + 31) / 32) * 4, hipMemcpyDeviceToHost, p->copy);
    if (e == hipSuccess) e = hipEventRecord(s.hcopied[k], p->copy);
    err[g] = e;
  }
}

// the whole batch on the CPU backend (a CPU context; the fallback of a GPU one)
void cpu_call(at2v_ctx* ctx, const HostBatch& b) {
  if (b.transfers) {
    at2v::cpu_verify_transfers(ctx->cpu, b.pk, b.sig, b.recipient, b.amount, b.n, b.wire, (int)ctx->policy, b.verdicts);
    if (b.recipient_ok) at2v::cpu_decode_points(ctx->cpu, b.recipient, b.n, b.recipient_ok);
  } else {
    at2v::cpu_verify_batch(ctx->cpu, b.pk, b.sig, b.msg, b.msg_off, b.n, (int)ctx->policy, b.verdicts);
  }
  ++ctx->cpu_batches;
}

// every stream a host-buffer call enqueued work on is idle: nothing of it can land in the caller's arrays any more
void drain_shard_streams(at2v_ctx* ctx) {
  for (Shard& s : ctx->shards) {
    if (hipSetDevice(s.device) != hipSuccess) continue;
    (void)hipStreamSynchronize(s.stream);
    if (s.pipe) sync_pipe_streams(*s.pipe);
  }
}

// Complete slot k's call: wait for its verdict copies (not for the cache builds behind them); on a device error with
// AT2V_CTX_CPU_FALLBACK, drain and verify the batch on the CPU (the caller's buffers are still valid: the call has not
// returned to the caller as complete).
void host_call_finish(at2v_ctx* ctx, int k) {
  HostCall& hc = ctx->calls[k];
  if (!hc.active || hc.done) return;
  int rc = AT2V_OK;
  for (size_t g = 0; g < ctx->shards.size(); ++g)
    if (hc.m[g] && hc.err[g] != hipSuccess && rc == AT2V_OK) rc = hip_code(hc.err[g]);
  for (size_t g = 0; g < ctx->shards.size(); ++g) {
    Shard& s = ctx->shards[g];
    if (hc.m[g] == 0 || hc.err[g] != hipSuccess || hipSetDevice(s.device) != hipSuccess) continue;
    hipError_t e = hipEventSynchronize(s.hcopied[k]);
    if (e != hipSuccess && rc == AT2V_OK) rc = hip_code(e);
  }
  if (ctx->pipe_trace)
    std::fprintf(stderr, "[at2v pipe] n %zu: %.3f ms (host: wait %.3f, copy %.3f, enqueue %.3f ms)\n", hc.b.n,
                 std::chrono::duration<double>(std::chrono::steady_clock::now() - hc.t0).count() * 1e3,
                 ctx->tr_wait * 1e3, ctx->tr_copy * 1e3, ctx->tr_enq * 1e3);
  if (rc != AT2V_OK && ctx->cpu) {
    // AT2V_CTX_CPU_FALLBACK: the records are still in the caller's host buffers. Drain what the shards enqueued (no
    // verdict copy of this call may land after the CPU's words), then verify the whole batch on the CPU backend.
    drain_shard_streams(ctx);
    cpu_call(ctx, hc.b);
    ++ctx->cpu_fallbacks;
    rc = AT2V_OK;
  }
  if (rc != AT2V_OK) {
    // a host-buffer call fails closed: once nothing of it can land any more, every word of its outputs is 0 (also when a
    // later submit completes the call and its result code is lost)
    drain_shard_streams(ctx);
    const size_t words = (hc.b.n + 31) / 32;
    std::memset(hc.b.verdicts, 0, words * 4);
    if (hc.b.recipient_ok) std::memset(hc.b.recipient_ok, 0, words * 4);
  }
  hc.rc = rc;
  hc.done = true;
}

// complete every host-buffer call still in flight (their results stay for at2v_verify_batch_wait)
void drain_host_calls(at2v_ctx* ctx) {
  const DeviceScope keep;
  for (uint64_t t = ctx->next_ticket > 2 ? ctx->next_ticket - 2 : 1; t < ctx->next_ticket; ++t)
    if (ctx->calls[t % 2].ticket == t) host_call_finish(ctx, (int)(t % 2));
}

// Before a pinned host range goes away (or a preload changes the sender cache): the host-buffer calls in flight complete
// (their results stay for their waits), and every upload a failed call may have left behind has landed, so no DMA reads
// the range any more.
void quiesce_host_calls(at2v_ctx* ctx) {
  if (ctx->shards.empty()) return;
  drain_host_calls(ctx);
  for (Shard& s : ctx->shards)
    if (s.pipe) wait_all_uploads(*s.pipe);
}

int host_call_check(at2v_ctx* ctx, const HostBatch& b) {
  if (!ctx) return AT2V_E_INVALID;
  if (b.transfers) {  // the wire first: also for n = 0
    if (at2v::transfer_msg_len(b.wire) == 0) return AT2V_E_INVALID;
    if (b.n && (!b.pk || !b.sig || !b.recipient || !b.amount || !b.verdicts || b.n >= (1u << 31))) return AT2V_E_INVALID;
    return AT2V_OK;
  }
  if (b.n == 0) return AT2V_OK;
  if (!b.pk || !b.sig || !b.msg_off || !b.verdicts || b.n >= (1u << 31)) return AT2V_E_INVALID;
  if (!b.msg && b.msg_off[b.n] != b.msg_off[0]) return AT2V_E_INVALID;
  if (!at2v::offsets_valid(b.msg_off, b.n)) return AT2V_E_INVALID;  // whole batch, before any device work
  return AT2V_OK;
}

// a fresh call in slot hc: active, not done, over the caller's arrays
void begin_host_call(HostCall& hc, const HostBatch& b) {
  hc = HostCall{};
  hc.active = true;
  hc.b = b;
}

// the two halves and the synchronous form, for a records call and a transfers call alike
int host_call_submit(at2v_ctx* ctx, const HostBatch& b, uint64_t* ticket) {
  if (!ticket) return AT2V_E_INVALID;
  *ticket = 0;
  const size_t n = b.n;
  const int chk = host_call_check(ctx, b);
  if (chk != AT2V_OK) return chk;
  const uint64_t t = ctx->next_ticket++;
  const int k = (int)(t % 2);
  HostCall& hc = ctx->calls[k];
  const DeviceScope keep;
  host_call_finish(ctx, k);  // the call two tickets back: its slot's bitmaps and arenas are reused (its result is lost
                             // unless waited for; at most two calls are in flight)
  begin_host_call(hc, b);
  hc.ticket = t;
  *ticket = t;
  if (n == 0) {
    hc.done = true;
  } else if (ctx->shards.empty()) {  // CPU context: verified now
    cpu_call(ctx, b);
    hc.done = true;
  } else {
    host_call_issue(ctx, k);
  }
  return AT2V_OK;
}

int host_call_sync(at2v_ctx* ctx, const HostBatch& b) {
  const int chk = host_call_check(ctx, b);
  if (chk != AT2V_OK || b.n == 0) return chk;
  if (ctx->shards.empty()) {  // CPU context
    cpu_call(ctx, b);
    return AT2V_OK;
  }
  const DeviceScope keep;
  drain_host_calls(ctx);
  HostCall& hc = ctx->calls[2];
  begin_host_call(hc, b);
  host_call_issue(ctx, 2);
  host_call_finish(ctx, 2);
  hc.active = false;
  return hc.rc;
}

HostBatch transfers_batch(const uint8_t* sender, const uint8_t* sig, const uint8_t* recipient, const uint64_t* amount,
                          size_t n, int wire, uint32_t* verdicts, uint32_t* recipient_ok) {
  HostBatch b{sender, sig, nullptr, nullptr, n, verdicts};
  b.transfers = true;
  b.recipient = recipient;
  b.amount = amount;
  b.wire = wire;
  b.recipient_ok = recipient_ok;
  return b;
}

}  // namespace

int at2v_verify_batch_submit(at2v_ctx* ctx, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                             const uint32_t* msg_off, size_t n, uint32_t* verdicts, uint64_t* ticket) {
  return host_call_submit(ctx, HostBatch{pk, sig, msg, msg_off, n, verdicts}, ticket);
}

int at2v_verify_batch_wait(at2v_ctx* ctx, uint64_t ticket) {
  if (!ctx || ticket == 0 || ticket >= ctx->next_ticket) return AT2V_E_INVALID;
  HostCall& hc = ctx->calls[ticket % 2];
  if (hc.ticket != ticket || !hc.active) return AT2V_E_INVALID;  // already waited for, or two or more calls back
  const DeviceScope keep;
  host_call_finish(ctx, (int)(ticket % 2));
  hc.active = false;
  return hc.rc;
}

int at2v_verify_batch(at2v_ctx* ctx, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg,
                      const uint32_t* msg_off, size_t n, uint32_t* verdicts) {
  return host_call_sync(ctx, HostBatch{pk, sig, msg, msg_off, n, verdicts});
}

int at2v_verify_transfers(at2v_ctx* ctx, const uint8_t* sender, const uint8_t* sig, const uint8_t* recipient,
                          const uint64_t* amount, size_t n, int wire, uint32_t* verdicts, uint32_t* recipient_ok) {
  return host_call_sync(ctx, transfers_batch(sender, sig, recipient, amount, n, wire, verdicts, recipient_ok));
}

int at2v_verify_transfers_submit(at2v_ctx* ctx, const uint8_t* sender, const uint8_t* sig, const uint8_t* recipient,
                                 const uint64_t* amount, size_t n, int wire, uint32_t* verdicts,
                                 uint32_t* recipient_ok, uint64_t* ticket) {
  return host_call_submit(ctx, transfers_batch(sender, sig, recipient, amount, n, wire, verdicts, recipient_ok), ticket);
}
