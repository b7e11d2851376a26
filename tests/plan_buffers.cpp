// The owning arena of the solver plans (csrc/plan_buffers.hpp, device-free) over counting fakes of the device layer, built with
// -fsanitize=address,undefined by tests/test_plan_buffers.py.  The script below has the shape of cgnr_create_impl: required
// blocks, one optional marked group (resident mode), more required blocks, and after "create" one lazily added group that is
// all-or-none (the staging of rls_cgnr_solve_queue_host).  Every allocation of it is made to fail in turn.  Leaks and double
// frees are the sanitizer's to catch; the counts are checked here.
#include "../regularizedleastsquares.jl_amd/csrc/plan_buffers.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#define CHECK(cond)                                                                       \
  do {                                                                                    \
    if (!(cond)) {                                                                        \
      fprintf(stderr, "FAILED (fail_at = %d) %s:%d: %s\n", g_fail_at, __FILE__, __LINE__, #cond); \
      exit(1);                                                                            \
    }                                                                                     \
  } while (0)

static int g_fail_at = 0;  // the ordinal (1-based, device and pinned requests counted together) of the request that fails; 0 = none

struct fake_device {
  int requests = 0;                  // allocation calls that reached the device layer
  std::map<void*, bool> live;        // block -> pinned?
  std::vector<void*> alloc_order, free_order, zeroed;
  int zero_fail_code = 0;            // the next zero-fill request fails with this

  int alloc(void** p, size_t bytes, bool pinned) {
    if (++requests == g_fail_at) return 700 + requests;
    *p = malloc(bytes);
    memset(*p, 0xA5, bytes);
    live[*p] = pinned;
    alloc_order.push_back(*p);
    return 0;
  }
  void free_(void* p, bool pinned) {
    auto it = live.find(p);
    if (it == live.end() || it->second != pinned) {
      fprintf(stderr, "FAILED (fail_at = %d): free of a block that is not live, or through the wrong callable\n", g_fail_at);
      exit(1);
    }
    live.erase(it);
    free_order.push_back(p);
    free(p);
  }
  int zero(void* p, size_t bytes) {
    if (zero_fail_code) return zero_fail_code;
    memset(p, 0, bytes);
    zeroed.push_back(p);
    return 0;
  }
  plan_buffers arena() {
    return plan_buffers([this](void** p, size_t n) { return alloc(p, n, false); }, [this](void* p) { free_(p, false); },
                        [this](void** p, size_t n) { return alloc(p, n, true); }, [this](void* p) { free_(p, true); },
                        [this](void* p, size_t n) { return zero(p, n); });
  }
};

static bool all_bytes(const void* p, size_t n, unsigned char v) {
  const unsigned char* q = static_cast<const unsigned char*>(p);
  return std::all_of(q, q + n, [v](unsigned char c) { return c == v; });
}

struct plan {
  float* a = nullptr;      // dev, zeroed
  int* b_h = nullptr;      // pinned, zeroed
  void* c = nullptr;       // dev
  void* sync = nullptr;    // optional group: dev
  unsigned* flags_h = nullptr;  // optional group: pinned, zeroed
  double* f = nullptr;     // dev, zeroed
  void* g = nullptr;       // dev
  void* q_b = nullptr;     // lazy group: dev
  char* q_bh = nullptr;    // lazy group: pinned
  char* q_xh = nullptr;    // lazy group: pinned
};
constexpr int N_CREATE = 7, N_ALL = 10;

static bool lazy_group(plan_buffers& mem, plan& P) {
  const plan_buffers::mark_t m = mem.mark();
  mem.dev(&P.q_b, 96, false);
  mem.pinned(&P.q_bh, 96, false);
  mem.pinned(&P.q_xh, 48, false);
  if (!mem.error()) return true;
  mem.rollback(m);
  return false;
}

static void run(int fail_at) {
  g_fail_at = fail_at;
  fake_device D;
  plan P;
  plan_buffers mem = D.arena();
  std::vector<void*> want_zeroed;  // device blocks marked `zero` that were handed out

  // ---- "create" ----
  mem.dev(&P.a, 64, true);
  mem.pinned(&P.b_h, 32, true);
  mem.dev(&P.c, 128, false);
  bool optional = false;
  if (!mem.error()) {
    const plan_buffers::mark_t m = mem.mark();
    mem.dev(&P.sync, 256, false);
    mem.pinned(&P.flags_h, 16, true);
    optional = !mem.error();
    if (!optional) {
      const size_t before = D.free_order.size();
      const int in_group = fail_at - 4;  // blocks of the group handed out before the failure
      CHECK(fail_at == 4 || fail_at == 5);
      CHECK(mem.error() == 700 + fail_at);
      mem.rollback(m);
      CHECK(D.free_order.size() - before == (size_t)in_group);  // exactly the group
      CHECK(!P.sync && !P.flags_h);                              // ... its pointers nulled
      CHECK(mem.error() == 0);                                   // ... and its error forgotten
      CHECK(P.a && P.b_h && P.c && D.live.size() == 3);          // what came before the mark is untouched
    }
  }
  mem.dev(&P.f, 80, true);
  mem.dev(&P.g, 8, false);
  const bool required_failed = fail_at >= 1 && fail_at <= N_CREATE && !(fail_at == 4 || fail_at == 5);
  CHECK((mem.error() != 0) == required_failed);

  if (required_failed) {
    CHECK(mem.error() == 700 + fail_at);  // the first error, not a later one
    CHECK(D.requests == fail_at);         // nothing reached the device layer after it
    mem.fail(999);
    CHECK(mem.error() == 700 + fail_at);  // sticky
    CHECK((int)D.live.size() == fail_at - 1);
  } else {
    CHECK(D.requests == (fail_at == 4 ? N_CREATE - 1 : N_CREATE));  // (the group's second request was a no-op behind the first's failure)
    // ---- after "create": the lazily added group, all three or none ----
    bool lazy = lazy_group(mem, P);
    if (fail_at > N_CREATE) {
      CHECK(!lazy && mem.error() == 0);
      CHECK(!P.q_b && !P.q_bh && !P.q_xh);
      CHECK(D.free_order.size() == (size_t)(fail_at - N_CREATE - 1));  // exactly the group's blocks
      CHECK((int)D.live.size() == N_CREATE);
      lazy = lazy_group(mem, P);  // the next call starts from nothing and succeeds
    }
    CHECK(lazy && P.q_b && P.q_bh && P.q_xh);
    CHECK(all_bytes(P.q_bh, 96, 0xA5) && all_bytes(P.q_xh, 48, 0xA5) && all_bytes(P.q_b, 96, 0xA5));  // not marked: untouched
    CHECK((int)D.live.size() == (optional ? N_ALL : N_ALL - 2));
  }

  // ---- zero-fill: requested exactly for the blocks marked `zero` ----
  if (P.a) want_zeroed.push_back(P.a);
  if (P.f) want_zeroed.push_back(P.f);
  CHECK(D.zeroed == want_zeroed);
  if (P.b_h) CHECK(all_bytes(P.b_h, 32, 0));
  if (P.flags_h) CHECK(all_bytes(P.flags_h, 16, 0));
  if (P.c) CHECK(all_bytes(P.c, 128, 0xA5));
  if (P.sync) CHECK(all_bytes(P.sync, 256, 0xA5));
  if (P.g) CHECK(all_bytes(P.g, 8, 0xA5));

  // ---- "destroy": every live block exactly once, youngest first; a second release finds nothing ----
  std::vector<void*> want_order;
  for (void* p : D.alloc_order)
    if (D.live.count(p)) want_order.push_back(p);
  std::reverse(want_order.begin(), want_order.end());
  const size_t before = D.free_order.size();
  mem.release();
  CHECK(std::vector<void*>(D.free_order.begin() + before, D.free_order.end()) == want_order);
  CHECK(D.live.empty());
  CHECK(!P.a && !P.b_h && !P.c && !P.sync && !P.flags_h && !P.f && !P.g && !P.q_b && !P.q_bh && !P.q_xh);
  const size_t frees = D.free_order.size();
  mem.release();
  CHECK(D.free_order.size() == frees);
  CHECK(D.alloc_order.size() == frees);  // nothing handed out was left behind
}

// a zero-fill that cannot be enqueued is the request's failure; the block stays owned.  An arena that goes out of scope
// without release() frees what it holds.
static void run_zero_failure_and_scope_exit() {
  g_fail_at = 0;
  fake_device D;
  void *a = nullptr, *b = nullptr;
  {
    plan_buffers mem = D.arena();
    D.zero_fail_code = 55;
    mem.dev(&a, 64, true);
    CHECK(mem.error() == 55 && a && D.live.size() == 1);
    mem.dev(&b, 64, false);
    CHECK(!b && D.requests == 1);
  }
  CHECK(D.live.empty() && D.free_order.size() == 1);
}

int main() {
  for (int k = 0; k <= N_ALL; ++k) run(k);
  run_zero_failure_and_scope_exit();
  printf("plan buffers OK\n");
  return 0;
}
