// host_copy_map.h -- the check of a host map of pic_copy_envs.  No HIP in here: a pure function of the map and
// the two environment counts, compiled by tests/copy_map_driver.cpp with a plain host compiler.  The kernels of pic_copy.h
// hold a device map to the same rules, entry by entry (copy_source).
#pragma once

#include <cstdint>
#include <string>

// Empty: the map is good.  Otherwise what is wrong with it.  map: E_dst entries, or null (identity).
//   two handles: null needs E_dst == E_src; an entry e needs 0 <= map[e] < E_src
//   one handle (E_dst == E_src): null is refused; map[e] == e keeps e, every other entry must name a kept environment
//   (map[map[e]] == map[e]), so that no source is overwritten while it is read
static inline std::string check_copy_map(const int32_t* map, int E_dst, int E_src, bool same_handle) {
  if (!map) {
    if (same_handle) return "a copy inside one handle needs a map";
    if (E_dst != E_src)
      return "a null map is the identity and needs equal num_envs (" + std::to_string(E_dst) + " and " + std::to_string(E_src) + ")";
    return "";
  }
  for (int e = 0; e < E_dst; ++e) {
    const int32_t m = map[e];
    if (m < 0 || m >= E_src)
      return "map[" + std::to_string(e) + "] = " + std::to_string(m) + " is not an environment of the source (num_envs " +
             std::to_string(E_src) + ")";
    if (same_handle && m != e && map[m] != m)
      return "map[" + std::to_string(e) + "] = " + std::to_string(m) + " names an environment that is itself overwritten (map[" +
             std::to_string(m) + "] = " + std::to_string(map[m]) + "): a source must be kept";
  }
  return "";
}
