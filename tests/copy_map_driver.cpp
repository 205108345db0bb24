// The host map check of pic_copy_envs (csrc/host_copy_map.h) as a stand-alone program: host compiler, no HIP.  One case per
// input line: "E_dst E_src same_handle n m_0 .. m_{n-1}", n = -1 for a null map.  One output line per case: "ok", or
// "bad <reason>".
#include <cstdint>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "host_copy_map.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    int E_dst = 0, E_src = 0, same = 0, n = 0;
    if (!(in >> E_dst >> E_src >> same >> n)) continue;
    std::vector<int32_t> map(n > 0 ? n : 0);
    for (int i = 0; i < n; ++i) in >> map[i];
    if (n >= 0 && n != E_dst) { std::cout << "bad the driver wants E_dst entries\n"; continue; }
    const std::string r = check_copy_map(n < 0 ? nullptr : map.data(), E_dst, E_src, same != 0);
    std::cout << (r.empty() ? "ok" : "bad " + r) << "\n";
  }
  return 0;
}
