// at2v_cpu.h — the CPU batch backend of the product (at2v_opts.num_gpus = 0, and the opt-in fallback of a GPU context,
// AT2V_CTX_CPU_FALLBACK). It replaces the reference's SystemManager::run(.., num_cpus::get()) workers, which verify one
// payload each (/root/reference/src/bin/server/rpc.rs:124-125, the per-payload drop::crypto::sign check behind
// rpc.rs:275-284), with a pool of host threads over the SAME verify routine the GPU kernels run (verify_half_fu,
// at2v_verify_fu.h, compiled for the host in at2v_cpu.cpp): verdicts are identical by construction, and the oracle
// (oracle/) is never linked or called. Plain C++ declarations, so the hipcc-compiled context code can call them.
#pragma once
#include <cstddef>
#include <cstdint>

namespace at2v {

struct CpuPool;

// CPUs this process may run on: the affinity mask, capped by a cgroup v2/v1 CPU quota if one is set (a container that
// grants 16 of a host's 256 threads reports 256 in its mask).
unsigned usable_cpus();

// A pool of `threads` workers (0 = usable_cpus()); the calling thread of a batch works too, so `threads` - 1 are
// spawned. nullptr if no thread could be started.
CpuPool* cpu_pool_create(unsigned threads);
void cpu_pool_destroy(CpuPool* p);
unsigned cpu_pool_threads(const CpuPool* p);

// A pool without the verify tables, for host work of the GPU path (the staging copies of at2v_verify_batch), and its
// generic job: fn(arg, c) for c = 0..chunks-1 over the workers and the caller, synchronous. One job at a time per pool.
CpuPool* copy_pool_create(unsigned threads);
void pool_run(CpuPool* p, size_t chunks, void (*fn)(void*, size_t), void* arg);

// n records in the at2v_verify_batch layout -> ceil(n/32) verdict words (pad bits 0), synchronous. Chunks of 64 records
// own their two words, so workers never share a word. One batch at a time per pool (calls serialise).
void cpu_verify_batch(CpuPool* p, const uint8_t* pk, const uint8_t* sig, const uint8_t* msg, const uint32_t* msg_off,
                      size_t n, int policy, uint32_t* verdicts);

// The same over the fields of n transfers (at2v_verify_transfers): record i's message is built on the stack from
// recipient i and amount i (at2v_transfer.h; wire: AT2V_WIRE_BYTES or AT2V_WIRE_ARRAY, checked by the caller) and goes
// through the same verify routine. Whether the recipient decodes does not enter the verdict (cpu_decode_points tells).
void cpu_verify_transfers(CpuPool* p, const uint8_t* sender, const uint8_t* sig, const uint8_t* recipient,
                          const uint64_t* amount, size_t n, int wire, int policy, uint32_t* verdicts);

// bit i of valid_words = 1 iff pts[i] decodes under dalek rules (the kernels' gu_frombytes), synchronous
void cpu_decode_points(CpuPool* p, const uint8_t* pts, size_t n, uint32_t* valid_words);

// status[i] = AT2V_SENDER_BAD_KEY where pk[i] does not decode under dalek rules (gu_frombytes), else 0: what
// at2v_sender_preload / _query report beside the cache bits, and all they report on a context without a sender cache.
// Synchronous; p may be nullptr (a GPU context without a CPU pool: the calling thread decodes).
void cpu_sender_status(CpuPool* p, const uint8_t* pk, size_t n, uint8_t* status);

// reasons[i] = the at2v_reason of record i (at2v_reason.h reject_reason; 0 where bit i of verdict_words is set), n bytes,
// synchronous. policy: AT2V_POLICY_*. Chunks of 64 records own their bytes.
void cpu_reject_reasons(CpuPool* p, const uint8_t* pk, const uint8_t* sig, size_t n, const uint32_t* verdict_words,
                        int policy, uint8_t* reasons);

// mask[i] = the AT2V_MASK_* bits of record i (at2v_reason.h policy_mask; 0 where bit i of verdict_words, the verdicts of
// a verify under AT2V_POLICY_DALEK_V1_LEGACY, is clear), n bytes, synchronous. Chunks of 64 records own their bytes.
void cpu_policy_mask(CpuPool* p, const uint8_t* pk, const uint8_t* sig, size_t n, const uint32_t* verdict_words,
                     uint8_t* mask);

// One record through the joint-table form of the verify routine (verify_half_fu_joint, what the GPU's verify_kernel
// runs) with the host tables: the verdict at2v_verify_one_policy gives, 0 or 1. For tests (tests/host/joint_host.cpp);
// not part of the ABI. Arguments as at2v_verify_one_policy's, already checked.
int cpu_verify_one_joint(const uint8_t pk[32], const uint8_t sig[64], const uint8_t* msg, uint32_t len, int policy);

}  // namespace at2v
