// Standalone test of the sparse Update codec (wire.cpp: fields 2-4 of Update).  Host code only;
// meant to be built with -fsanitize=address,undefined and run directly:
//
//   g++ -std=c++17 -fsanitize=address,undefined -Icsrc/core csrc/core/test_wire_sparse.cpp \
//       csrc/core/wire.cpp -o test_wire_sparse && ./test_wire_sparse
//   -> prints "ok" and exits 0, or aborts on failure
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "wire.h"

#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::abort();                                                       \
    }                                                                     \
  } while (0)

using namespace slcore;

static std::vector<uint8_t> encode(const std::vector<uint32_t>& idx, const std::vector<float>& val, uint64_t n) {
  // exactly the computed size on the heap: a write past it is an ASan report
  std::vector<uint8_t> out(sparse_update_encoded_size(idx.size(), n));
  encode_sparse_update(idx.data(), val.data(), idx.size(), n, out.data());
  return out;
}

template <typename F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const WireError&) {
    return true;
  }
  return false;
}

static void golden() {
  // index [1, 5], value [1.0, -2.0], dense length 300
  const uint8_t want[] = {0x12, 0x08, 1, 0, 0, 0, 5, 0, 0, 0,
                          0x1a, 0x08, 0x00, 0x00, 0x80, 0x3f, 0x00, 0x00, 0x00, 0xc0,
                          0x20, 0xac, 0x02};
  const auto got = encode({1, 5}, {1.0f, -2.0f}, 300);
  CHECK(got.size() == sizeof(want) && std::memcmp(got.data(), want, sizeof(want)) == 0);
  CHECK(update_count(got.data(), got.size()) == 0);  // the dense parser sees an empty delta
  CHECK(encode({}, {}, 0).empty());
  const auto empty = encode({}, {}, 7);  // sparse, no entries
  const SparseView v = sparse_update_view(empty.data(), empty.size());
  CHECK(v.dense_len == 7 && sparse_update_validate(v) == 0);
}

static void roundtrip_and_fuzz() {
  std::mt19937_64 rng(11);
  for (int it = 0; it < 300; ++it) {
    const uint64_t n = 1 + rng() % 5000;
    std::vector<uint32_t> idx;
    std::vector<float> val;
    for (uint64_t i = 0; i < n; ++i)
      if (rng() % 7 == 0) {
        idx.push_back((uint32_t)i);
        val.push_back((float)(int64_t)(rng() % 2001 - 1000) / 64.f);
      }
    const auto msg = encode(idx, val, n);
    const SparseView v = sparse_update_view(msg.data(), msg.size());
    CHECK(v.dense_len == n);
    CHECK(sparse_update_validate(v) == idx.size());
    CHECK(idx.empty() || std::memcmp(v.index, idx.data(), 4 * idx.size()) == 0);
    CHECK(val.empty() || std::memcmp(v.value, val.data(), 4 * val.size()) == 0);
    // every truncation and random corruption either parses or throws WireError, never reads outside
    for (int cut = 0; cut < 8 && !msg.empty(); ++cut) {
      std::vector<uint8_t> bad(msg.begin(), msg.begin() + rng() % msg.size());
      try {
        sparse_update_validate(sparse_update_view(bad.data(), bad.size()));
      } catch (const WireError&) {
      }
      bad = msg;
      bad[rng() % bad.size()] ^= (uint8_t)(1u << (rng() % 8));
      try {
        sparse_update_validate(sparse_update_view(bad.data(), bad.size()));
      } catch (const WireError&) {
      }
    }
  }
}

static std::vector<uint8_t> raw_message(const std::string& index_bytes, const std::string& value_bytes, uint64_t n) {
  std::vector<uint8_t> out(64 + index_bytes.size() + value_bytes.size());
  uint8_t* p = out.data();
  *p++ = 0x12;
  p = put_varint(p, index_bytes.size());
  std::memcpy(p, index_bytes.data(), index_bytes.size());
  p += index_bytes.size();
  *p++ = 0x1a;
  p = put_varint(p, value_bytes.size());
  std::memcpy(p, value_bytes.data(), value_bytes.size());
  p += value_bytes.size();
  *p++ = 0x20;
  p = put_varint(p, n);
  out.resize((size_t)(p - out.data()));
  return out;
}

static std::string words(std::initializer_list<uint32_t> w) {
  std::string s;
  for (uint32_t x : w) s.append((const char*)&x, 4);
  return s;
}

static void rejections() {
  auto check = [](const std::vector<uint8_t>& m) { sparse_update_validate(sparse_update_view(m.data(), m.size())); };
  const std::string two_vals = words({0x3f800000u, 0x40000000u});
  CHECK(!throws([&] { check(raw_message(words({1, 2}), two_vals, 3)); }));
  CHECK(throws([&] { check(raw_message(words({1, 2}).substr(0, 7), two_vals, 3)); }));   // length % 4
  CHECK(throws([&] { check(raw_message(words({1, 2}), two_vals.substr(0, 6), 3)); }));
  CHECK(throws([&] { check(raw_message(words({1, 2, 3}), two_vals, 9)); }));              // unequal counts
  CHECK(throws([&] { check(raw_message(words({2, 2}), two_vals, 9)); }));                 // not strictly ascending
  CHECK(throws([&] { check(raw_message(words({2, 1}), two_vals, 9)); }));
  CHECK(throws([&] { check(raw_message(words({1, 3}), two_vals, 3)); }));                 // index >= sparse_len
  CHECK(throws([&] { check(raw_message(words({0xffffffffu, 0}), two_vals, ~0ull)); }));
}

int main() {
  golden();
  roundtrip_and_fuzz();
  rejections();
  std::puts("ok");
  return 0;
}
