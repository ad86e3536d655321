// cluster_parts_check.cpp — pbd::clusterParts (partsbaseddetector_amd/host/pbd_host.hpp) for tests/test_gpu_kmeans.py: def[P][n][2]
// doubles, parent[P] and K[P] int32 from files -> the labels, one line per part, and the capped count; then a refusal.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../partsbaseddetector_amd/host/pbd_host.hpp"

template <class T> static std::vector<T> slurp(const char* path) {
  std::vector<T> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  T x;
  while (fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 7) { printf("usage: cluster_parts_check def.bin parent.bin K.bin n R seed\n"); return 2; }
  const std::vector<double> def = slurp<double>(argv[1]);
  const std::vector<int32_t> parent = slurp<int32_t>(argv[2]);
  std::vector<int32_t> K = slurp<int32_t>(argv[3]);
  const int n = atoi(argv[4]), R = atoi(argv[5]);
  const uint64_t seed = strtoull(argv[6], nullptr, 10);
  try {
    int capped = -1;
    const std::vector<int32_t> idx = pbd::clusterParts(def, n, parent, K, R, seed, 1000, 0, &capped);
    for (size_t p = 0; p < parent.size(); ++p) {
      printf("part%zu", p);
      for (int i = 0; i < n; ++i) printf(" %d", idx[p * n + i]);
      printf("\n");
    }
    printf("capped %d\n", capped);
  } catch (const pbd::Exception& e) { printf("error %d %s\n", e.code, e.what()); return 1; }
  try {
    K[0] = PBD_CLUSTER_MAX_K + 1;
    pbd::clusterParts(def, n, parent, K, R, seed);
    printf("refused 0\n");
  } catch (const pbd::Exception& e) { printf("refused %d\n", e.code); }
  return 0;
}
