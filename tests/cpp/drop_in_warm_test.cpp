// MPC::setWarmStart of the drop-in header: the closed loop of the reference's src/test.cpp:79-111 (MPC::run once, then
// MPC::solve fed with its own step-1 state) twice from the same start, cold and warm-started.  Prints one line per solve and the
// iteration totals; tests/test_warm_start_gpu.py compares the two loops.  Exits with 3 when no GPU is present.
#include <cstdio>
#include <string>
#include <vector>

#include "mpc_drop_in.hpp"

int main(int argc, char **argv) {
  const std::string cfg = argc > 1 ? argv[1] : "../config-stable.json";
  const int steps = argc > 2 ? atoi(argv[2]) : 25;
  try {
    MPC mpc;
    Config::load(cfg);
    std::vector<double> ptsx = {-145.1165, -158.3417, -164.3164, -169.3365, -175.4917, -176.9617};
    std::vector<double> ptsy = {4.339378, -17.42898, -30.18062, -42.84062, -66.52898, -76.85062};
    Vehicle vehicle;
    vehicle.setLength(Config::Lf);
    vehicle.update(-146.7283, 1.660802, 4.125825, 26.6806, 0, 0);
    std::vector<double> vars = mpc.run(vehicle, ptsx, ptsy);
    const std::vector<double> start = {vars[0], vars[1], vars[2], vars[3], vars[6], vars[7]};
    for (int warm = 0; warm < 2; warm++) {
      mpc.setWarmStart(warm != 0);
      if (mpc.getWarmStart() != (warm != 0)) return 1;
      std::vector<double> state = start;
      long total = 0;
      for (int i = 0; i < steps; i++) {
        std::vector<double> v = mpc.solve(state, 40);
        printf("%s %d %d %.12g %.12g %.12g %.12g %.12g %.12g %.12g %.12g %.12g\n", warm ? "warm" : "cold", i, mpc.lastIterations(), v[0], v[1], v[2],
               v[3], v[4], v[5], v[6], v[7], v[8]);
        total += mpc.lastIterations();
        for (int k = 0; k < 6; k++) state[k] = v[k];
      }
      printf("%s total %ld\n", warm ? "warm" : "cold", total);
    }
  } catch (const std::string &e) {
    fprintf(stderr, "error: %s\n", e.c_str());
    return e.find("NO_DEVICE") != std::string::npos || e.find("no HIP device") != std::string::npos || e.find("mpc_create") != std::string::npos ? 3 : 1;
  }
  return 0;
}
