// shim_batch.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The drop-in claim of INTEGRATION.md at its smallest: include/rsbwt_gpubwt.hpp compiled against the reference's
// own headers, the reference's unmodified src/bwt/query.cpp searching through `const BWT*`, beside the shim's
// batched findIntervals.  Built by oracle/Makefile (`ref`) into oracle/_ref/shim_batch where the reference's sources
// are at hand, and run by tests/test_cpp_shim.py.
//
//   shim_batch <file.bwt> <k-mer>   prints: lower upper lower upper (findInterval, then the batch's second answer)
#include <iostream>
#include <memory>
#include "rsbwt_gpubwt.hpp"
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  try {
    GpuBWT* g = new GpuBWT(argv[1]);
    const BWT* pbwt = g;                              // the reference's abstract interface
    BWTInterval itv = findInterval(pbwt, argv[2]);    // the reference's own query.cpp
    std::vector<BWTInterval> b = findIntervals(g, {argv[2], argv[2]});
    std::cout << itv.lower << " " << itv.upper << " " << b[1].lower << " " << b[1].upper << "\n";
    delete g;
  } catch (const std::exception& e) {
    std::cout << "error: " << e.what() << "\n";
    return 3;
  }
  return 0;
}
