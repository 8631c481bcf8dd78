// at2v_reason_launch.h — the host-side entry point of the reject-reasons object (at2v_reason.hip), declared apart from
// at2v_launch.h so that the kernels object (at2v_kernels.hip) does not depend on it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace at2v {

// reasons[i] = the at2v_reason of record i for i < n (0 where bit i of verdict_words is set), asynchronous on `stream`.
// pk / sig / reasons 16-byte aligned; n < 2^31. Writes n bytes, none beyond.
// A weak symbol: a library linked from the context code without the reasons object (tests/test_experiment_guard.py links
// at2v_api.o with the kernels, host and CPU objects only) still loads; its reasons entry points then return
// hipErrorNoBinaryForGpu (AT2V_E_NODEVICE, "library built without the HIP kernels"), never a CPU answer.
__attribute__((weak)) hipError_t launch_reject_reasons(const uint8_t* pk, const uint8_t* sig, uint32_t n,
                                                       const uint32_t* verdict_words, uint8_t* reasons, int policy,
                                                       hipStream_t stream);

// mask[i] = the AT2V_MASK_* bits of record i for i < n (0 where bit i of verdict_words, the verdicts of a verify under
// the LEGACY policy, is clear), asynchronous on `stream`. Alignment, n and the bytes written as above; weak likewise.
__attribute__((weak)) hipError_t launch_policy_mask(const uint8_t* pk, const uint8_t* sig, uint32_t n,
                                                    const uint32_t* verdict_words, uint8_t* mask, hipStream_t stream);

}  // namespace at2v
