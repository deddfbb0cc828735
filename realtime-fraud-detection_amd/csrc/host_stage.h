// host_stage.h — device staging of a host (`_host`) entry point's batch (engine.hip). Not an ABI.
//
// Two steps, so that every argument check runs and the buffer has its final size before anything is queued: the entry
// point declares each column it moves — in(): host to device ahead of the launch, out(): device to host after it —
// then upload() lays the columns out in the engine's one staging buffer (Engine::stage; at most one reallocation,
// before any pointer into it exists), sets the typed device pointers the declarations named and queues the copies up.
// A null host pointer is an absent optional column: its device pointer becomes null and nothing is copied, which is
// how the kernels take an absent column too.
// Layout: every column starts on a kAlign boundary — what hipMalloc gave each of the separate buffers this replaces;
// text.hip's 16-byte loads need 16, no other kernel states a need — and kAlign bytes of padding end the buffer. No
// launch function reads a column past its count (the 16-byte loads of text.hip and ingest.hip stop at the last whole
// 16 bytes below the total and finish byte by byte).
// The buffer is shared by every host entry point and ordered by e.stream alone, as the buffers before it were.
#pragma once

#include <cstring>

#include "fd_internal.h"

namespace fd {

class Stage {
 public:
  explicit Stage(Engine& e) : e_(e) {}
  template <class T>
  void in(const T*& dev, const T* host, size_t count) { add(&dev, const_cast<T*>(host), count * sizeof(T), true); }
  template <class T>
  void out(T*& dev, T* host, size_t count) { add(&dev, host, count * sizeof(T), false); }
  void upload() {
    e_.stage.ensure(total_ + kAlign);
    for (int k = 0; k < n_; ++k) {
      const Seg& s = segs_[k];
      void* d = s.host ? e_.stage.as<char>() + s.off : nullptr;
      std::memcpy(s.dev, &d, sizeof(d));  // (*s.dev is a T* of the declaration's type)
      if (s.up && d && s.bytes) FD_HIP(hipMemcpyAsync(d, s.host, s.bytes, hipMemcpyHostToDevice, e_.stream));
    }
  }
  // the declared outputs to the host; wait: then until e.stream has drained
  void download(bool wait = true) {
    for (int k = 0; k < n_; ++k) {
      const Seg& s = segs_[k];
      if (!s.up && s.host && s.bytes)
        FD_HIP(hipMemcpyAsync(s.host, e_.stage.as<char>() + s.off, s.bytes, hipMemcpyDeviceToHost, e_.stream));
    }
    if (wait) FD_HIP(hipStreamSynchronize(e_.stream));
  }

 private:
  static constexpr size_t kAlign = 256;
  static constexpr int kMaxSegs = 24;  // fd_ingest_json_host: 2 inputs + the 20 columns of fd_ingest_out
  struct Seg {
    void* dev;  // the caller's device pointer variable
    void* host;
    size_t bytes, off;
    bool up;
  };
  void add(void* dev, void* host, size_t bytes, bool up) {
    FD_REQUIRE(n_ < kMaxSegs, FD_ERR_INVALID_ARG, "internal: too many staged columns");
    segs_[n_++] = Seg{dev, host, bytes, total_, up};
    if (host) total_ = (total_ + bytes + kAlign - 1) / kAlign * kAlign;
  }
  Engine& e_;
  Seg segs_[kMaxSegs];
  int n_ = 0;
  size_t total_ = 0;
};

// The columns of fd_txn_batch an entry point stages, as bits in the struct's order
enum : unsigned { kTxnKey = 1, kTxnTs = 2, kTxnCents = 4, kTxnMerchant = 8, kTxnAll = 0xFF };

inline void stage_txns(Stage& st, fd_txn_batch& dev, const fd_txn_batch& host, int64_t n, unsigned cols) {
  unsigned bit = 1;
  auto col = [&](auto member) {
    if (cols & bit) st.in(dev.*member, host.*member, (size_t)n);
    bit <<= 1;
  };
  col(&fd_txn_batch::card_key);
  col(&fd_txn_batch::ts_ms);
  col(&fd_txn_batch::amount_cents);
  col(&fd_txn_batch::merchant);
  col(&fd_txn_batch::device_fp);
  col(&fd_txn_batch::ip_class);
  col(&fd_txn_batch::hour);
  col(&fd_txn_batch::weekend);
}

}  // namespace fd
