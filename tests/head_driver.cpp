// head_driver.cpp -- the part of csrc/host_head.h that needs no HIP, as a stand-alone program for tests/test_head_cpu.py: the
// parameter count and the shape check that the MLP policy's and the particle actor's calls share.
// stdin: one row per line,  max_layers n_layers w0 .. w7 layernorm mem_kind activation squash per_env has_params.
// stdout: one line each: "P=<head_param_count> <head_bad_shape's message, or ok>".  The caller's own checks say nothing here.
#include <cstdio>

#include "host_head.h"

struct Spec {      // the fields of pic_policy and pic_actor that the shape check reads, with room for the widths of 7 layers
  int n_layers, width[8], activation, squash, per_env;
  const double* params;
};

int main() {
  static const double some = 0.0;
  char line[256];
  while (std::fgets(line, sizeof line, stdin)) {
    Spec s{};
    int max_layers, layernorm, mem_kind, has_params;
    int* const w = s.width;
    if (std::sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &max_layers, &s.n_layers, w, w + 1, w + 2, w + 3, w + 4,
                    w + 5, w + 6, w + 7, &layernorm, &mem_kind, &s.activation, &s.squash, &s.per_env, &has_params) != 16 ||
        s.n_layers < 0 || s.n_layers > 7) {
      std::fprintf(stderr, "head_driver: malformed line: %s", line);
      return 2;
    }
    s.params = has_params ? &some : nullptr;
    const char* bad = head_bad_shape(s, mem_kind, max_layers, [](int) -> const char* { return nullptr; });
    std::printf("P=%zu %s\n", head_param_count(s.width, s.n_layers, layernorm != 0), bad ? bad : "ok");
  }
  return 0;
}
