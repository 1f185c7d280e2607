// Prints the work tables of protosam_amd/csrc/work_tables.h for the shapes on its command line: the real C++ the launchers upload,
// compiled by tests/test_work_tables_cpu.py with the host compiler and its sanitizers. No HIP, no library.
// Every argument is kind:a:b:... and gives one line "kind a b ... | grid rows | words" (or "... | refused"):
//   tile_map:ntm:ntn:mode              word per block of tile_map_grid: tm | tn << 16, -1 where the block has no tile
//   pick_map_mode:ntm:ntn:cus:xcds     one word, the mode
//   splitk_ranges:M:N:K:ncu            one word, the number of K ranges
//   gemm_table:ntm:ntn:mode:G   splitk_table:ntm:ntn:mode:ks:G   gattn_table:BH:nqb:xcds   wattn_worklist:B:H:grid   wattn_geometry:rs2
#include "../protosam_amd/csrc/work_tables.h"
#include <stdio.h>
#include <stdlib.h>
#include <string>

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    std::string s(argv[i]), label(s);
    for (auto& ch : label) if (ch == ':') ch = ' ';
    size_t p = s.find(':');
    const std::string kind = s.substr(0, p);
    long long a[5] = {0, 0, 0, 0, 0};
    int n = 0;
    while (p != std::string::npos && n < 5) {
      const size_t q = s.find(':', p + 1);
      a[n++] = atoll(s.substr(p + 1, q == std::string::npos ? q : q - p - 1).c_str());
      p = q;
    }
    WorkTable t;
    if (kind == "tile_map") {
      t.grid = tile_map_grid((int)a[0], (int)a[1], (int)a[2]);
      for (int b = 0; b < t.grid; ++b) {
        int tm = 0, tn = 0;
        t.words.push_back(tile_map(b, (int)a[0], (int)a[1], (int)a[2], tm, tn) ? tm | (tn << 16) : -1);
      }
    } else if (kind == "pick_map_mode") t.words.push_back(pick_map_mode((int)a[0], (int)a[1], (int)a[2], (int)a[3]));
    else if (kind == "splitk_ranges") t.words.push_back(splitk_ranges((int)a[0], (int)a[1], (int)a[2], (int)a[3]));
    else if (kind == "gemm_table") t = gemm_work_table((int)a[0], (int)a[1], (int)a[2], (int)a[3]);
    else if (kind == "splitk_table") t = splitk_work_table((int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)a[4]);
    else if (kind == "gattn_table") t = gattn_work_table((int)a[0], (int)a[1], (int)a[2]);
    else if (kind == "wattn_worklist") t = wattn_work_list((int)a[0], (int)a[1], (int)a[2]);
    else if (kind == "wattn_geometry") t = wattn_geometry_table(a[0]);
    else { fprintf(stderr, "unknown table kind in %s\n", argv[i]); return 2; }
    if (t.words.empty()) { printf("%s | refused\n", label.c_str()); continue; }
    printf("%s | %d %d |", label.c_str(), t.grid, t.rows);
    for (int w : t.words) printf(" %d", w);
    printf("\n");
  }
  return 0;
}
