// Test driver for cmx::Mica::analyse with nullMethod = "permutations" on an alphabet other than 4 / 20 states
// (include/comap_mi355x_adapter.hpp), model-free.
//   adapter_mica_perm_main <input.bin>  -> output.file (cmx::io::writeMica) on stdout
// input.bin: int32 T, N, S, maxNbPermutations, firstCoordinate; uint64 seed; uint8 aln[T][N]
#include <cstdio>
#include <fstream>
#include <iostream>

#include "comap_mi355x_adapter.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::cerr << "usage: adapter_mica_perm_main <input.bin>\n";
    return 2;
  }
  try {
    std::ifstream in(argv[1], std::ios::binary);
    int32_t h[5];
    uint64_t seed;
    in.read(reinterpret_cast<char*>(h), sizeof(h));
    in.read(reinterpret_cast<char*>(&seed), sizeof(seed));
    const size_t T = h[0], N = h[1];
    std::vector<uint8_t> aln(T * N);
    in.read(reinterpret_cast<char*>(aln.data()), aln.size());
    if (!in) throw cmx::Exception("input file too short");
    cmx::Engine eng(0);
    cmx::Mica::Options opt;
    opt.nullMethod = "permutations";
    opt.maxNbPermutations = h[3];
    opt.seed = seed;
    const cmx::Mica::Result res = cmx::Mica::analyse(eng, aln.data(), T, N, h[2], nullptr, 0, nullptr, opt);
    std::vector<int> coords(N);
    for (size_t i = 0; i < N; ++i) coords[i] = h[4] + (int)i;
    cmx::io::writeMica(res, coords, std::cout);
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << "\n";
    return 1;
  }
  return 0;
}
