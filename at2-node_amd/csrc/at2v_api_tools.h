// at2v_api_tools.h — the entry points beside the verify path: the record generator, the signer, point decoding and the
// reject reasons and the policy mask (part of the one translation unit at2v_api.hip). Each works on the context's first
// shard.
#pragma once
#include "at2v_api_ctx.h"
#include "at2v_reason_launch.h"

namespace {

int gen_records(at2v_ctx* ctx, uint64_t cfg_seed, uint64_t first, size_t n, uint32_t msg_len, uint64_t senders,
                const uint64_t* d_keys, uint8_t* d_pk, uint8_t* d_sig, uint8_t* d_msg, uint32_t* d_msg_off,
                void* hip_stream) {
  if (!ctx) return AT2V_E_INVALID;
  if (n == 0) return AT2V_OK;
  if (!d_pk || !d_sig || (!d_msg && msg_len) || n >= (1u << 31) || (uint64_t)n * msg_len >= (1ull << 32))
    return AT2V_E_INVALID;
  if (ctx->shards.empty()) return AT2V_E_NODEVICE;
  if (!aligned(d_pk, 4) || !aligned(d_sig, 4) || (d_msg_off && !aligned(d_msg_off, 4)) || !aligned(d_keys, 8))
    return AT2V_E_ALIGN;
  const DeviceScope scope(ctx->shards[0].device);
  hipError_t e = scope.err;
  if (e == hipSuccess)
    e = at2v::launch_gen(cfg_seed, first, (uint32_t)n, msg_len, senders, d_keys, d_pk, d_sig, d_msg, d_msg_off,
                         (hipStream_t)hip_stream);
  return hip_code(e);
}

// The reject-reasons launch of a context (current device = the shard's). It takes no scratch set and records no event:
// the pass reads only the caller's records and verdict words, so it orders nothing but its own stream.
hipError_t launch_reasons(at2v_ctx* ctx, const uint8_t* d_pk, const uint8_t* d_sig, size_t n,
                          const uint32_t* d_verdicts, uint8_t* d_reasons, hipStream_t stream) {
  if (ctx->test_fail_launches) {  // test hook (AT2V_TEST_FAIL_LAUNCH): a launch failure, as a faulting device reports it
    --ctx->test_fail_launches;
    return hipErrorLaunchFailure;
  }
  if (!at2v::launch_reject_reasons) return hipErrorNoBinaryForGpu;  // linked without at2v_reason.o (a weak symbol)
  return at2v::launch_reject_reasons(d_pk, d_sig, (uint32_t)n, d_verdicts, d_reasons, (int)ctx->policy, stream);
}

// The policy-mask launch of a context, as launch_reasons: no scratch set, no event, no sender cache.
hipError_t launch_mask(at2v_ctx* ctx, const uint8_t* d_pk, const uint8_t* d_sig, size_t n, const uint32_t* d_verdicts,
                       uint8_t* d_mask, hipStream_t stream) {
  if (ctx->test_fail_launches) {
    --ctx->test_fail_launches;
    return hipErrorLaunchFailure;
  }
  if (!at2v::launch_policy_mask) return hipErrorNoBinaryForGpu;  // linked without at2v_reason.o (a weak symbol)
  return at2v::launch_policy_mask(d_pk, d_sig, (uint32_t)n, d_verdicts, d_mask, stream);
}

// The host form on a GPU context: every record travels (an accepted record's mask depends on its bytes, a rejected one's
// is 0), with the caller's verdict words; the n bytes come back into `mask`.
hipError_t mask_of_records(at2v_ctx* ctx, Shard& s, const uint8_t* pk, const uint8_t* sig, size_t n,
                           const uint32_t* verdicts, uint8_t* mask) {
  const size_t words = (n + 31) / 32;
  const DeviceScope scope(s.device);
  hipError_t e = scope.err;
  if (e == hipSuccess) e = s.pk.ensure(n * 32);
  if (e == hipSuccess) e = s.sig.ensure(n * 64);
  if (e == hipSuccess) e = s.verdict.ensure(words * 4);
  if (e == hipSuccess) e = s.reasons.ensure(n);
  if (e == hipSuccess) e = hipMemcpyAsync(s.pk.p, pk, n * 32, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(s.sig.p, sig, n * 64, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(s.verdict.p, verdicts, words * 4, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess)
    e = launch_mask(ctx, (const uint8_t*)s.pk.p, (const uint8_t*)s.sig.p, n, (const uint32_t*)s.verdict.p,
                    (uint8_t*)s.reasons.p, s.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(mask, s.reasons.p, n, hipMemcpyDeviceToHost, s.stream);
  const hipError_t es = s.stream ? hipStreamSynchronize(s.stream) : hipSuccess;  // (also after an error)
  return e != hipSuccess ? e : es;
}

// The host form on a GPU context: only the m rejected records (idx, ascending) go to the device, with an all-zero
// verdict array; their reason bytes come back into `got`.
hipError_t reasons_of_rejects(at2v_ctx* ctx, Shard& s, const uint8_t* pk, const uint8_t* sig,
                              const std::vector<uint32_t>& idx, std::vector<uint8_t>& got) {
  const size_t m = idx.size(), words = (m + 31) / 32;
  std::vector<uint8_t> gpk(m * 32), gsig(m * 64);
  for (size_t k = 0; k < m; ++k) {
    std::memcpy(&gpk[k * 32], pk + (size_t)idx[k] * 32, 32);
    std::memcpy(&gsig[k * 64], sig + (size_t)idx[k] * 64, 64);
  }
  got.assign(m, AT2V_REASON_UNKNOWN);
  const DeviceScope scope(s.device);
  hipError_t e = scope.err;
  if (e == hipSuccess) e = s.pk.ensure(m * 32);
  if (e == hipSuccess) e = s.sig.ensure(m * 64);
  if (e == hipSuccess) e = s.verdict.ensure(words * 4);
  if (e == hipSuccess) e = s.reasons.ensure(m);
  if (e == hipSuccess) e = hipMemcpyAsync(s.pk.p, gpk.data(), m * 32, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(s.sig.p, gsig.data(), m * 64, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess) e = hipMemsetAsync(s.verdict.p, 0, words * 4, s.stream);
  if (e == hipSuccess)
    e = launch_reasons(ctx, (const uint8_t*)s.pk.p, (const uint8_t*)s.sig.p, m, (const uint32_t*)s.verdict.p,
                       (uint8_t*)s.reasons.p, s.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(got.data(), s.reasons.p, m, hipMemcpyDeviceToHost, s.stream);
  // (also after an error: the pageable source arrays of the uploads die with this frame)
  const hipError_t es = s.stream ? hipStreamSynchronize(s.stream) : hipSuccess;
  return e != hipSuccess ? e : es;
}

}  // namespace

int at2v_gen_records_device(at2v_ctx* ctx, uint64_t cfg_seed, uint64_t first, size_t n, uint32_t msg_len,
                            uint8_t* d_pk, uint8_t* d_sig, uint8_t* d_msg, uint32_t* d_msg_off, void* hip_stream) {
  return gen_records(ctx, cfg_seed, first, n, msg_len, 0, nullptr, d_pk, d_sig, d_msg, d_msg_off, hip_stream);
}

int at2v_gen_records_senders_device(at2v_ctx* ctx, uint64_t cfg_seed, uint64_t first, size_t n, uint32_t msg_len,
                                    uint64_t senders, uint8_t* d_pk, uint8_t* d_sig, uint8_t* d_msg,
                                    uint32_t* d_msg_off, void* hip_stream) {
  return gen_records(ctx, cfg_seed, first, n, msg_len, senders, nullptr, d_pk, d_sig, d_msg, d_msg_off, hip_stream);
}

int at2v_gen_records_keys_device(at2v_ctx* ctx, uint64_t cfg_seed, uint64_t first, size_t n, uint32_t msg_len,
                                 const uint64_t* d_keys, uint8_t* d_pk, uint8_t* d_sig, uint8_t* d_msg,
                                 uint32_t* d_msg_off, void* hip_stream) {
  if (n && !d_keys) return AT2V_E_INVALID;
  return gen_records(ctx, cfg_seed, first, n, msg_len, 0, d_keys, d_pk, d_sig, d_msg, d_msg_off, hip_stream);
}

int at2v_sign_batch(at2v_ctx* ctx, const uint8_t* seeds, const uint8_t* msg, const uint32_t* msg_off, size_t n,
                    uint8_t* pk_out, uint8_t* sig_out) {
  if (!ctx) return AT2V_E_INVALID;
  if (n == 0) return AT2V_OK;
  if (!seeds || !msg_off || !pk_out || !sig_out || n >= (1u << 31)) return AT2V_E_INVALID;
  if (ctx->shards.empty()) return AT2V_E_NODEVICE;  // (signing is the client's side, not the verify path)
  Shard& s = ctx->shards[0];
  const uint32_t mb0 = msg_off[0], mb1 = msg_off[n];
  if (mb1 < mb0 || (!msg && mb1 != mb0)) return AT2V_E_INVALID;
  const size_t mbytes = mb1 - mb0;
  std::vector<uint32_t> offs(n + 1);
  for (size_t i = 0; i <= n; ++i) {
    offs[i] = msg_off[i] - mb0;
    if (i && offs[i] < offs[i - 1]) return AT2V_E_INVALID;
  }
  const DeviceScope scope(s.device);
  DevBuf dseed, dmsg, doff, dpk, dsig;
  hipError_t e = scope.err;
  if (e == hipSuccess) e = dseed.ensure(n * 32);
  if (e == hipSuccess) e = dmsg.ensure(mbytes + 16);
  if (e == hipSuccess) e = doff.ensure((n + 1) * 4);
  if (e == hipSuccess) e = dpk.ensure(n * 32);
  if (e == hipSuccess) e = dsig.ensure(n * 64);
  if (e == hipSuccess) e = hipMemcpyAsync(dseed.p, seeds, n * 32, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess && mbytes) e = hipMemcpyAsync(dmsg.p, msg + mb0, mbytes, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(doff.p, offs.data(), (n + 1) * 4, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess)
    e = at2v::launch_sign((const uint8_t*)dseed.p, (const uint8_t*)dmsg.p, (uint32_t)mbytes, (const uint32_t*)doff.p,
                          (uint32_t)n, (uint8_t*)dpk.p, (uint8_t*)dsig.p, s.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(pk_out, dpk.p, n * 32, hipMemcpyDeviceToHost, s.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(sig_out, dsig.p, n * 64, hipMemcpyDeviceToHost, s.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  for (DevBuf* b : {&dseed, &dmsg, &doff, &dpk, &dsig}) b->release();
  return hip_code(e);
}

int at2v_decode_points(at2v_ctx* ctx, const uint8_t* pts, size_t n, uint32_t* valid_words) {
  if (!ctx) return AT2V_E_INVALID;
  if (n == 0) return AT2V_OK;
  if (!pts || !valid_words || n >= (1u << 31)) return AT2V_E_INVALID;
  if (ctx->shards.empty()) {  // CPU context: the kernels' decode routine on the host
    at2v::cpu_decode_points(ctx->cpu, pts, n, valid_words);
    return AT2V_OK;
  }
  Shard& s = ctx->shards[0];
  const DeviceScope scope(s.device);
  const size_t words = (n + 31) / 32;
  hipError_t e = scope.err;
  if (e == hipSuccess) e = s.pk.ensure(n * 32);
  if (e == hipSuccess) e = s.verdict.ensure(words * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(s.pk.p, pts, n * 32, hipMemcpyHostToDevice, s.stream);
  if (e == hipSuccess) e = at2v::launch_decode((const uint8_t*)s.pk.p, (uint32_t)n, (uint32_t*)s.verdict.p, s.stream);
  if (e == hipSuccess) e = hipMemcpyAsync(valid_words, s.verdict.p, words * 4, hipMemcpyDeviceToHost, s.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s.stream);
  return hip_code(e);
}

int at2v_reject_reasons_device(at2v_ctx* ctx, const uint8_t* d_pk, const uint8_t* d_sig, size_t n,
                               const uint32_t* d_verdicts, uint8_t* d_reasons, void* hip_stream) {
  if (!ctx) return AT2V_E_INVALID;
  if (n == 0) return AT2V_OK;
  if (!d_pk || !d_sig || !d_verdicts || !d_reasons || n >= (1u << 31)) return AT2V_E_INVALID;
  if (ctx->shards.empty()) return AT2V_E_NODEVICE;
  if (!aligned(d_pk, 16) || !aligned(d_sig, 16) || !aligned(d_verdicts, 4) || !aligned(d_reasons, 16))
    return AT2V_E_ALIGN;
  const DeviceScope scope(ctx->shards[0].device);
  hipError_t e = scope.err;
  if (e == hipSuccess) e = launch_reasons(ctx, d_pk, d_sig, n, d_verdicts, d_reasons, (hipStream_t)hip_stream);
  return hip_code(e);
}

int at2v_reject_reasons(at2v_ctx* ctx, const uint8_t* pk, const uint8_t* sig, size_t n, const uint32_t* verdicts,
                        uint8_t* reasons) {
  if (!ctx) return AT2V_E_INVALID;
  if (n == 0) return AT2V_OK;
  if (!reasons || n >= (1u << 31)) return AT2V_E_INVALID;
  if (!pk || !sig || !verdicts) {
    std::memset(reasons, AT2V_REASON_UNKNOWN, n);
    return AT2V_E_INVALID;
  }
  if (ctx->shards.empty()) {  // CPU context: the same routine over its thread pool
    at2v::cpu_reject_reasons(ctx->cpu, pk, sig, n, verdicts, (int)ctx->policy, reasons);
    return AT2V_OK;
  }
  // valid records get their 0 here; only the rejected ones travel (a 1M batch with 10 % rejects uploads 10 MB, not 96)
  std::vector<uint32_t> idx;
  std::vector<uint8_t> got;
  int rc = AT2V_OK;
  try {
    for (size_t w = 0; w < (n + 31) / 32; ++w) {
      const size_t left = n - 32 * w;
      uint32_t rej = ~verdicts[w] & (left >= 32 ? 0xffffffffu : (1u << left) - 1u);  // pad bits are not rejects
      for (; rej; rej &= rej - 1) idx.push_back((uint32_t)(32 * w) + (uint32_t)__builtin_ctz(rej));
    }
    std::memset(reasons, AT2V_REASON_VALID, n);
    if (idx.empty()) return AT2V_OK;
    rc = hip_code(reasons_of_rejects(ctx, ctx->shards[0], pk, sig, idx, got));
  } catch (const std::bad_alloc&) {
    rc = AT2V_E_OOM;
  }
  if (rc == AT2V_OK) {
    for (size_t k = 0; k < idx.size(); ++k) reasons[idx[k]] = got[k];
    return AT2V_OK;
  }
  if (ctx->cpu) {  // AT2V_CTX_CPU_FALLBACK: the records are still on the host
    at2v::cpu_reject_reasons(ctx->cpu, pk, sig, n, verdicts, (int)ctx->policy, reasons);
    return AT2V_OK;
  }
  std::memset(reasons, AT2V_REASON_UNKNOWN, n);  // fail closed
  return rc;
}

int at2v_policy_mask_device(at2v_ctx* ctx, const uint8_t* d_pk, const uint8_t* d_sig, size_t n,
                            const uint32_t* d_verdicts, uint8_t* d_mask, void* hip_stream) {
  if (!ctx || ctx->policy != AT2V_POLICY_DALEK_V1_LEGACY) return AT2V_E_INVALID;
  if (n == 0) return AT2V_OK;
  if (!d_pk || !d_sig || !d_verdicts || !d_mask || n >= (1u << 31)) return AT2V_E_INVALID;
  if (ctx->shards.empty()) return AT2V_E_NODEVICE;
  if (!aligned(d_pk, 16) || !aligned(d_sig, 16) || !aligned(d_verdicts, 4) || !aligned(d_mask, 16)) return AT2V_E_ALIGN;
  const DeviceScope scope(ctx->shards[0].device);
  hipError_t e = scope.err;
  if (e == hipSuccess) e = launch_mask(ctx, d_pk, d_sig, n, d_verdicts, d_mask, (hipStream_t)hip_stream);
  return hip_code(e);
}

int at2v_policy_mask(at2v_ctx* ctx, const uint8_t* pk, const uint8_t* sig, size_t n, const uint32_t* verdicts,
                     uint8_t* mask) {
  if (!ctx || ctx->policy != AT2V_POLICY_DALEK_V1_LEGACY) return AT2V_E_INVALID;  // nothing written
  if (n == 0) return AT2V_OK;
  if (!mask || n >= (1u << 31)) return AT2V_E_INVALID;
  if (!pk || !sig || !verdicts) {
    std::memset(mask, 0, n);
    return AT2V_E_INVALID;
  }
  if (ctx->shards.empty()) {  // CPU context: the same routine over its thread pool
    at2v::cpu_policy_mask(ctx->cpu, pk, sig, n, verdicts, mask);
    return AT2V_OK;
  }
  const int rc = hip_code(mask_of_records(ctx, ctx->shards[0], pk, sig, n, verdicts, mask));
  if (rc == AT2V_OK) return AT2V_OK;
  if (ctx->cpu) {  // AT2V_CTX_CPU_FALLBACK: the records are still on the host
    at2v::cpu_policy_mask(ctx->cpu, pk, sig, n, verdicts, mask);
    return AT2V_OK;
  }
  std::memset(mask, 0, n);  // fail closed: no policy accepts
  return rc;
}
