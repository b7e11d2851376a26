// The one owner of a solver plan's device and pinned-host blocks (plans.hpp and the files that include it, plans_f64.hip).  Free of any device API, as
// host_pool.hpp is, so that it also compiles with plain g++ under -fsanitize=address,undefined (tests/plan_buffers.cpp, run by
// tests/test_plan_buffers.py): the device layer enters only through the five callables it is constructed with.
//
// A create function asks for its blocks one after the other and looks at error() once: after the first failure every
// later request is a no-op.  Blocks a plan can do without are asked for between mark() and, on failure, rollback().  The
// plan's destroy function calls release() and names no block.
#pragma once
#include <cstddef>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

struct plan_buffers {
  using alloc_fn = std::function<int(void** p, size_t bytes)>;  // 0, or the device layer's own status
  using free_fn = std::function<void(void* p)>;
  using zero_fn = std::function<int(void* p, size_t bytes)>;  // enqueue the zero-fill of a device block on the plan's stream

  struct mark_t {
    size_t blocks;
    int err;
  };

  plan_buffers(alloc_fn dev_alloc, free_fn dev_free, alloc_fn pinned_alloc, free_fn pinned_free, zero_fn dev_zero)
      : dev_alloc_(std::move(dev_alloc)), dev_free_(std::move(dev_free)), pinned_alloc_(std::move(pinned_alloc)),
        pinned_free_(std::move(pinned_free)), dev_zero_(std::move(dev_zero)) {}
  plan_buffers(const plan_buffers&) = delete;
  plan_buffers& operator=(const plan_buffers&) = delete;
  ~plan_buffers() { release(); }

  // a device block behind *p (which must live as long as the arena: a member of the plan); `zero`: its zero-fill goes on the
  // stream right behind the allocation
  template <typename T>
  void dev(T** p, size_t bytes, bool zero) {
    if (err_) return;
    void* q = nullptr;
    const int status = dev_alloc_(&q, bytes);
    if (note(status, q, reinterpret_cast<void**>(p), false) && zero) fail(dev_zero_(q, bytes));
  }
  // the same in pinned host memory (zeroed by the host, at once)
  template <typename T>
  void pinned(T** p, size_t bytes, bool zero) {
    if (err_) return;
    void* q = nullptr;
    const int status = pinned_alloc_(&q, bytes);
    if (note(status, q, reinterpret_cast<void**>(p), true) && zero) memset(q, 0, bytes);
  }
  // a failure of the device layer on the way (a zero-fill that could not be enqueued) counts as a failed request
  void fail(int status) {
    if (!err_) err_ = status;
  }
  int error() const { return err_; }  // the FIRST failure: later ones do not overwrite it

  mark_t mark() const { return {blocks_.size(), err_}; }
  // back to the state at `m`: frees what was handed out since (youngest first), nulls those pointers, forgets a failure raised since
  void rollback(mark_t m) {
    while (blocks_.size() > m.blocks) {
      const block b = blocks_.back();
      blocks_.pop_back();
      (b.is_pinned ? pinned_free_ : dev_free_)(b.p);
      *b.slot = nullptr;
    }
    err_ = m.err;
  }
  // every block, exactly once, in reverse order of allocation; a second call finds nothing to free
  void release() { rollback({0, err_}); }

 private:
  struct block {
    void** slot;
    void* p;
    bool is_pinned;
  };
  bool note(int status, void* q, void** slot, bool is_pinned) {
    if (status != 0 || !q) {
      err_ = status != 0 ? status : -1;
      return false;
    }
    blocks_.push_back({slot, q, is_pinned});
    *slot = q;
    return true;
  }
  alloc_fn dev_alloc_;
  free_fn dev_free_;
  alloc_fn pinned_alloc_;
  free_fn pinned_free_;
  zero_fn dev_zero_;
  std::vector<block> blocks_;
  int err_ = 0;
};
