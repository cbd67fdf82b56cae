// Stand-alone host program (tests/test_objfields_host.py builds it with the address and undefined-behaviour sanitizers): the
// argument rules of cnr_obj_train / cnr_obj_workspace_bytes (csrc/obj_args.h) on a real argument set -- buffers of exactly the
// sizes the header documents -- and on every way of getting it wrong.  Nothing is launched: this is the code that runs before.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "obj_args.h"

using namespace cnr_obj;

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

int main() {
  const int N = 3, R = 120, n1 = 3, n2 = 7, S = n1 + n2, P = 11363;
  const int64_t lens[N] = {250, 400, 1000};
  std::vector<int64_t> pool_off(N + 1, 0);
  for (int o = 0; o < N; ++o) pool_off[o + 1] = pool_off[o] + lens[o];
  const int64_t rows = pool_off[N];
  std::vector<uint8_t> rgbs(rows * 4);
  std::vector<float> depth(rows), dirs(rows * 3), T(rows * 16), theta((size_t)N * P), m((size_t)N * P), v((size_t)N * P), losses(3 * N);
  std::vector<int64_t> state(N * 4);
  std::vector<int32_t> flags(N);
  std::vector<int> prow((size_t)N * R);
  std::vector<float> u((size_t)N * R * S), g((size_t)N * R * n2);
  // the workspace: its size from the query, every object's block inside it, 16-byte aligned
  const int64_t wsb = workspace_bytes(N, R, S);
  EXPECT(wsb == N * ws_words(R, S) * 4 && ws_words(R, S) % 4 == 0);
  EXPECT(ws_words(R, S) * 4 >= (int64_t)(8 * R * S + 5 * R) * 4 + 2 * R);
  void* ws = std::aligned_alloc(16, (size_t)wsb);
  std::memset(ws, 0, (size_t)wsb);
  for (int o = 0; o < N; ++o) {                       // the last byte of every object's block, as the kernel lays it out
    uint8_t* base = static_cast<uint8_t*>(ws) + (size_t)o * ws_words(R, S) * 4;
    uint8_t* labels = base + (size_t)(8 * R * S + 5 * R) * 4 + R;
    labels[R - 1] = 1;
  }
  int64_t shortest = lens[0];
  for (int o = 1; o < N; ++o) shortest = lens[o] < shortest ? lens[o] : shortest;
  const Required ok{rgbs.data(), depth.data(), dirs.data(), T.data(), pool_off.data(), state.data(), theta.data(), m.data(), v.data(),
                    losses.data(), flags.data(), ws};
  EXPECT(check_args(ok, shortest, N, R, n1, n2, 2.0f, nullptr, nullptr, nullptr, wsb) == 0);
  EXPECT(check_args(ok, shortest, N, R, n1, n2, 2.0f, prow.data(), u.data(), g.data(), wsb) == 0);
  // every refusal
  EXPECT(check_args(ok, shortest, N, R, 8, 57, 2.0f, nullptr, nullptr, nullptr, INT64_MAX) == E_ARG);        // S = 65
  EXPECT(check_args(ok, shortest, N, R, 2147483647, 2147483647, 2.0f, nullptr, nullptr, nullptr, INT64_MAX) == E_ARG);   // no overflow
  EXPECT(check_args(ok, shortest, 0, R, n1, n2, 2.0f, nullptr, nullptr, nullptr, wsb) == E_ARG);             // N = 0
  EXPECT(check_args(ok, shortest, -1, R, n1, n2, 2.0f, nullptr, nullptr, nullptr, wsb) == E_ARG);
  EXPECT(check_args(ok, shortest, N, 0, n1, n2, 2.0f, nullptr, nullptr, nullptr, wsb) == E_ARG);
  EXPECT(check_args(ok, R - 1, N, R, n1, n2, 2.0f, nullptr, nullptr, nullptr, wsb) == E_ARG);                // a pool shorter than R
  EXPECT(check_args(ok, shortest, N, 251, n1, n2, 2.0f, nullptr, nullptr, nullptr, INT64_MAX) == E_ARG);
  EXPECT(check_args(ok, shortest, N, R, -1, n2, 2.0f, nullptr, nullptr, nullptr, wsb) == E_ARG);
  EXPECT(check_args(ok, shortest, N, R, n1, 0, 2.0f, nullptr, nullptr, nullptr, wsb) == E_ARG);
  EXPECT(check_args(ok, shortest, N, R, n1, n2, 0.0f, nullptr, nullptr, nullptr, wsb) == E_ARG);
  EXPECT(check_args(ok, shortest, N, R, n1, n2, 2.0f, prow.data(), nullptr, nullptr, wsb) == E_ARG);         // a partial parity set
  EXPECT(check_args(ok, shortest, N, R, n1, n2, 2.0f, prow.data(), u.data(), nullptr, wsb) == E_ARG);
  EXPECT(check_args(ok, shortest, N, R, n1, n2, 2.0f, nullptr, u.data(), g.data(), wsb) == E_ARG);
  EXPECT(check_args(ok, shortest, N, R, n1, n2, 2.0f, nullptr, nullptr, nullptr, wsb - 1) == E_ARG);         // a short workspace
  Required bad = ok;
  bad.workspace = static_cast<uint8_t*>(ws) + 4;                                                             // misaligned
  EXPECT(check_args(bad, shortest, N, R, n1, n2, 2.0f, nullptr, nullptr, nullptr, wsb - 4) == E_ARG);
  const void** fields = reinterpret_cast<const void**>(&bad);
  for (size_t i = 0; i < sizeof(Required) / sizeof(void*); ++i) {                                           // each required pointer
    bad = ok;
    fields[i] = nullptr;
    EXPECT(check_args(bad, shortest, N, R, n1, n2, 2.0f, nullptr, nullptr, nullptr, wsb) == E_ARG);
  }
  EXPECT(workspace_bytes(0, R, S) == E_ARG && workspace_bytes(N, 0, S) == E_ARG && workspace_bytes(N, R, 65) == E_ARG &&
         workspace_bytes(N, R, 0) == E_ARG);
  EXPECT(workspace_bytes(100000, 100000, 64) == 100000ll * ws_words(100000, 64) * 4);                      // 64-bit arithmetic
  EXPECT(workspace_bytes(2147483647, 2147483647, 64) == E_ARG);                                              // ... and its end
  std::free(ws);
  if (failures) return 1;
  std::printf("ok obj_args\n");
  return 0;
}
