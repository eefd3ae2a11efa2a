// internal.hpp -- helpers shared by the C++ host layer (not installed).
#pragma once
#include <hip/hip_runtime_api.h>

#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "warpdb/csv_loader.hpp"
#include "warpexec.h"

namespace warpdb {

inline void hip_ok(hipError_t e, const char *what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP error: ") + what + ": " + hipGetErrorString(e));
}

class DevGuard {
 public:
  explicit DevGuard(int dev) {
    if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
    if (prev_ != dev) hip_ok(hipSetDevice(dev), "hipSetDevice");
    dev_ = dev;
  }
  ~DevGuard() {
    if (prev_ >= 0 && prev_ != dev_) (void)hipSetDevice(prev_);
  }

 private:
  int prev_ = -1, dev_ = 0;
};

// RAII device allocation.
struct DeviceBuffer {
  void *ptr = nullptr;
  int device = 0;
  DeviceBuffer() = default;
  DeviceBuffer(int dev, size_t bytes) : device(dev) {
    DevGuard g(dev);
    hip_ok(hipMalloc(&ptr, bytes ? bytes : 1), "hipMalloc");
  }
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
  DeviceBuffer(DeviceBuffer &&o) noexcept : ptr(o.ptr), device(o.device) { o.ptr = nullptr; }
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
    std::swap(ptr, o.ptr);
    std::swap(device, o.device);
    return *this;
  }
  ~DeviceBuffer() {
    if (ptr) {
      DevGuard g(device);
      (void)hipFree(ptr);
    }
  }
  void *release() {
    void *p = ptr;
    ptr = nullptr;
    return p;
  }
};

// A wx_table view over a Table's columns (names kept alive here).
struct WxTableView {
  explicit WxTableView(const Table &t);
  std::vector<std::string> names;
  std::vector<wx_col> cols;
  wx_table table{};
};

// Host <-> HBM copies (transfer.cpp).  copy_h2d may return before the DMA
// finishes (the source is already staged); copy_d2h returns with `dst` filled.
void copy_h2d(int device, hipStream_t s, void *dst, const void *src, size_t bytes);
void copy_d2h(int device, hipStream_t s, void *dst, const void *src, size_t bytes);
// A zero-filled host result of n floats (huge-page backed when large).
std::vector<float> host_result(size_t n);

// CSV data rows in [b, e) appended to `out` (typed columns already set up),
// parsed on up to `threads` threads (csv_parse.cpp).
int parse_threads();  // $WARPDB_PARSE_THREADS, default hardware threads, at most 16
void parse_csv_rows(const char *b, const char *e, HostTable &out, int threads);

// Headerless CSV text cut into tables of rows_per_chunk rows (the last one
// shorter), every column Float32 as in the reference's chunk loader
// (src/csv_loader.cpp:186-223).  The text is read in blocks of `block` bytes
// and each chunk is cut after its rows_per_chunk-th non-empty line with
// memchr (line-by-line std::getline capped the streaming pipeline at
// ≈29-41 M rows/s); a chunk's rows are parsed on parse_threads() threads.
class CsvChunkReader {
 public:
  CsvChunkReader(std::istream &in, std::vector<std::string> names, int64_t rows_per_chunk,
                 size_t block = size_t(64) << 20)
      : in_(in), names_(std::move(names)), rows_per_chunk_(rows_per_chunk), block_(block) {}
  // The next chunk (never empty) into `chunk`; false once the input is exhausted.
  bool next(HostTable &chunk);

 private:
  std::istream &in_;
  const std::vector<std::string> names_;
  const int64_t rows_per_chunk_;
  const size_t block_;
  std::string buf_;   // the unconsumed text: buf_[start_..)
  size_t start_ = 0;
  bool eof_ = false, done_ = false;
};

wx_launch sync_launch(int device, void *stream = nullptr);
void throw_on(wx_status st, const char *err);

// One C ABI call: fn(args..., err, sizeof(err)) with the error buffer every
// wx_* signature ends in, and throw_on of its status.
template <typename Fn, typename... Args>
void wx_call(Fn fn, Args &&...args) {
  char err[8192];
  throw_on(fn(std::forward<Args>(args)..., err, sizeof(err)), err);
}

}  // namespace warpdb
