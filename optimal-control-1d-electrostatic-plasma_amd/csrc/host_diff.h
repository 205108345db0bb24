// host_diff.h -- shared by host_phase.h, host_tape.h and host_tangent.h; included by picstep.hip alone, behind its helpers
#pragma once

// A device block cut into parts, every part rounded up to 256 bytes.  A block is described once, by a function that take()s its
// parts in order into the views of a holder and returns `at`, the block's bytes (tape_parts, tape_kl_parts, tangent_parts): with
// base = null and a scratch holder it only sizes the block, with the block's address it assigns the views.  A part without
// elements gets no view (null).
struct Carver {
  char* base = nullptr;
  size_t at = 0;
  static size_t rounded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  template <typename T>
  void take(T*& view, size_t count) {
    if (base) view = count ? reinterpret_cast<T*>(base + at) : nullptr;
    at += rounded(count * sizeof(T));
  }
  // bytes of consecutive parts: from the start of the first to `end`, the end of the last one's elements, rounded
  static size_t upto(const void* first, const void* end) {
    return rounded((size_t)(static_cast<const char*>(end) - static_cast<const char*>(first)));
  }
};

// the kind of a copy to or from the caller's memory: `host_kind` for PIC_HOST, else device to device
inline hipMemcpyKind copy_kind(int mem_kind, hipMemcpyKind host_kind) {
  return mem_kind == PIC_HOST ? host_kind : hipMemcpyDeviceToDevice;
}

// rows of device memory from the caller's src in mem_kind's memory, or zeros for a null src
inline hipError_t device_fill(pic_handle* h, double* dst, const double* src, size_t bytes, int mem_kind) {
  return src ? hipMemcpyAsync(dst, src, bytes, copy_kind(mem_kind, hipMemcpyHostToDevice), h->stream) : hipMemsetAsync(dst, 0, bytes, h->stream);
}

// An input in device memory: src itself when it is device memory (or null), else its copy in `buf`, the caller's device memory
inline hipError_t device_input(pic_handle* h, const double* src, int kind, size_t bytes, double* buf, const double** out) {
  *out = src;
  if (!src || kind == PIC_DEVICE) return hipSuccess;
  *out = buf;
  return hipMemcpyAsync(buf, src, bytes, hipMemcpyHostToDevice, h->stream);
}

// Device memory for an output: dst itself when it is device memory (or null), else `buf`; device_result copies it to dst behind
// the kernels that wrote it
inline double* device_output(void* dst, int kind, double* buf) { return dst && kind == PIC_HOST ? buf : static_cast<double*>(dst); }
inline hipError_t device_result(pic_handle* h, void* dst, const double* dev, size_t bytes) {
  return dst && dev != dst ? hipMemcpyAsync(dst, dev, bytes, hipMemcpyDeviceToHost, h->stream) : hipSuccess;
}

// argument checks of the pic_tape_* entries
inline int check_mem_kind(pic_handle* h, int mem_kind, const char* who) {
  return mem_kind == PIC_HOST || mem_kind == PIC_DEVICE ? PIC_OK : fail(h, PIC_EINVAL, std::string(who) + ": bad mem_kind");
}
inline int check_tape_open(pic_handle* h, const char* who) {
  return h->tape.on ? PIC_OK : fail(h, PIC_ESTATE, std::string(who) + ": no tape is open (pic_tape_start)");
}
// `what`, an argument that was given, needs the tape's a-bar rows
inline int check_tape_actuator(pic_handle* h, const void* given, const char* what, const char* who) {
  if (!given || h->tape.gact) return PIC_OK;
  return fail(h, PIC_ESTATE, std::string(who) + ": " + what + " needs an actuator set before pic_tape_start (pic_set_actuator)");
}
