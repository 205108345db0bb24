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

// argument checks of the pic_tape_* entries
inline int check_mem_kind(pic_handle* h, int mem_kind, const char* who) {
  return mem_kind == PIC_HOST || mem_kind == PIC_DEVICE ? PIC_OK : fail(h, PIC_EINVAL, std::string(who) + ": bad mem_kind");
}
inline int check_tape_open(pic_handle* h, const char* who) {
  return h->tape.on ? PIC_OK : fail(h, PIC_ESTATE, std::string(who) + ": no tape is open (pic_tape_start)");
}
// the forward-mode entries that take no parameter direction stop at steps under an MLP policy (pic_tape_step_policy): their
// actions depend on the state through the network; pic_tape_tangent_policy (host_tangent_walk.h) is the entry for such a tape
inline int check_no_policy_steps(pic_handle* h, const char* who) {
  return h->tape.pcalls.empty() ? PIC_OK
                             : fail(h, PIC_EINVAL, std::string(who) + ": the tape holds steps of pic_tape_step_policy (policy steps are "
                                                                      "not built in forward mode)");
}
// `what`, an argument that was given, needs the tape's a-bar rows
inline int check_tape_actuator(pic_handle* h, const void* given, const char* what, const char* who) {
  if (!given || h->tape.gact) return PIC_OK;
  return fail(h, PIC_ESTATE, std::string(who) + ": " + what + " needs an actuator set before pic_tape_start (pic_set_actuator)");
}
