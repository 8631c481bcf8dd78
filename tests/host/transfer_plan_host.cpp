// transfer_plan_host.cpp — the HIP-free arithmetic of the transfers entry points on the host, under AddressSanitizer +
// UBSan (tests/test_transfer_plan_host.py builds and runs it): a program of its own.
//   msg     at2v_transfer.h: the signed message of a transfer from (recipient, amount, wire), bytes and words, against
//           literal bytes for both wires and the amounts 0, 1 and 2^64 - 1; nothing written past the message
// (A transfers chunk's layout, uploads and arena bound are checked beside the records form's: stage_plan_host.cpp, tplan.)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "at2v_transfer.h"

namespace {

[[noreturn]] void fail(const char* what, size_t a = 0, size_t b = 0, size_t c = 0, size_t d = 0) {
  std::printf("FAIL %s: %zu %zu %zu %zu\n", what, a, b, c, d);
  std::exit(1);
}

// recipient bytes 0xa0 .. 0xbf
const uint8_t kRecipient[32] = {0xa0, 0xa1, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
                                0xab, 0xac, 0xad, 0xae, 0xaf, 0xb0, 0xb1, 0xb2, 0xb3, 0xb4, 0xb5,
                                0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xbb, 0xbc, 0xbd, 0xbe, 0xbf};
#define AT2V_T_RECIPIENT                                                                                              \
  0xa0, 0xa1, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xab, 0xac, 0xad, 0xae, 0xaf, 0xb0, 0xb1, 0xb2,   \
      0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xbb, 0xbc, 0xbd, 0xbe, 0xbf
#define AT2V_T_LEN32 0x20, 0, 0, 0, 0, 0, 0, 0

struct MsgCase {
  uint64_t amount;
  uint8_t bytes48[48];  // AT2V_WIRE_BYTES
  uint8_t array40[40];  // AT2V_WIRE_ARRAY
};
const MsgCase kCases[] = {
    {0ull, {AT2V_T_LEN32, AT2V_T_RECIPIENT, 0, 0, 0, 0, 0, 0, 0, 0}, {AT2V_T_RECIPIENT, 0, 0, 0, 0, 0, 0, 0, 0}},
    {1ull, {AT2V_T_LEN32, AT2V_T_RECIPIENT, 1, 0, 0, 0, 0, 0, 0, 0}, {AT2V_T_RECIPIENT, 1, 0, 0, 0, 0, 0, 0, 0}},
    {0xffffffffffffffffull,
     {AT2V_T_LEN32, AT2V_T_RECIPIENT, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff},
     {AT2V_T_RECIPIENT, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff, 0xff}},
    // every amount byte distinct: the byte order is little-endian
    {0x0807060504030201ull,
     {AT2V_T_LEN32, AT2V_T_RECIPIENT, 1, 2, 3, 4, 5, 6, 7, 8},
     {AT2V_T_RECIPIENT, 1, 2, 3, 4, 5, 6, 7, 8}},
};

int run_msg() {
  size_t cases = 0;
  if (at2v::transfer_msg_len(at2v::kTransferWireBytes) != 48 || at2v::transfer_msg_len(at2v::kTransferWireArray) != 40)
    fail("message length");
  for (int bad : {-1, 2, 3, 1 << 20})
    if (at2v::transfer_msg_len(bad) != 0) fail("a wire that is neither has a length", (size_t)bad);
  uint32_t rw[8];
  for (int k = 0; k < 8; ++k)
    rw[k] = (uint32_t)kRecipient[4 * k] | (uint32_t)kRecipient[4 * k + 1] << 8 | (uint32_t)kRecipient[4 * k + 2] << 16 |
            (uint32_t)kRecipient[4 * k + 3] << 24;
  for (const MsgCase& c : kCases)
    for (int wire : {at2v::kTransferWireBytes, at2v::kTransferWireArray}) {
      const uint8_t* want = wire == at2v::kTransferWireBytes ? c.bytes48 : c.array40;
      const uint32_t len = at2v::transfer_msg_len(wire);
      // bytes, into a heap buffer of exactly `len` + a guard the sanitizer also watches
      uint8_t* out = static_cast<uint8_t*>(std::malloc(len));
      if (!out) fail("malloc");
      if (at2v::transfer_msg_bytes(out, kRecipient, c.amount, wire) != len) fail("bytes: length", (size_t)wire);
      if (std::memcmp(out, want, len) != 0) fail("bytes differ from the literal", (size_t)wire, (size_t)c.amount);
      std::free(out);
      // words: the little-endian words of the same bytes, and no word past them
      uint32_t w[at2v::kTransferMaxWords];
      for (uint32_t& x : w) x = 0xEEEEEEEEu;
      if (at2v::transfer_msg_words(w, rw, c.amount, wire) != len) fail("words: length", (size_t)wire);
      for (uint32_t k = 0; k < len / 4; ++k) {
        const uint32_t ww = (uint32_t)want[4 * k] | (uint32_t)want[4 * k + 1] << 8 | (uint32_t)want[4 * k + 2] << 16 |
                            (uint32_t)want[4 * k + 3] << 24;
        if (w[k] != ww) fail("word differs from the literal", (size_t)wire, k, w[k], ww);
      }
      for (uint32_t k = len / 4; k < at2v::kTransferMaxWords; ++k)
        if (w[k] != 0xEEEEEEEEu) fail("word written past the message", (size_t)wire, k);
      ++cases;
    }
  std::printf("cases %zu\n", cases);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!std::strcmp(mode, "msg")) return run_msg();
  std::fprintf(stderr, "usage: %s msg\n", argv[0]);
  return 2;
}
