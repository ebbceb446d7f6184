// Walks csrc/hbk_mlp_gate.h (the train step's accumulation gate) on the CPU: built and run by
// tests/test_gate_rule.py as a child process with -fsanitize=address,undefined.
//
// stdin: one walk per line, the n_sel of its steps separated by blanks. Each walk starts from
// the state of a fresh epoch (acc_samples 0, acc_steps 1, t 0). stdout: per step one line
//   <walk> <step> <acc_samples> <acc_steps> <t> <fire> <scale as the float's bits in hex>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "hbk_mlp_gate.h"

int main() {
  std::string line;
  int walk = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    float acc_samples = 0.f, acc_steps = 1.f, t = 0.f, n_sel;
    int step = 0;
    while (in >> n_sel) {
      const hbk::StepGate g = hbk::step_gate(acc_samples, acc_steps, t, n_sel);
      uint32_t bits;
      static_assert(sizeof(bits) == sizeof(g.scale), "float bits");
      std::memcpy(&bits, &g.scale, sizeof(bits));
      std::printf("%d %d %.9g %.9g %.9g %.9g %08x\n", walk, step, g.acc_samples, g.acc_steps, g.adam_t, g.fire, bits);
      acc_samples = g.acc_samples;
      acc_steps = g.acc_steps;
      t = g.adam_t;
      ++step;
    }
    ++walk;
  }
  return 0;
}
