// MPC::setWarmStart on MPC::run() of the drop-in header: ten telemetry messages of one car (the scenario of the reference's
// src/test.cpp:45-50, the car moved on by an ideal plant to each solution's step-1 state) through run(), once with the warm start off
// and once, the same ten poses again, with it on.  Prints one line per call and the iteration totals; tests/test_run_warm_gpu.py
// compares the two.  Exits with 3 when no GPU is present.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "mpc_drop_in.hpp"

int main(int argc, char **argv) {
  const std::string cfg = argc > 1 ? argv[1] : "../config-stable.json";
  const int steps = argc > 2 ? atoi(argv[2]) : 10;
  try {
    MPC mpc;
    Config::load(cfg);
    const std::vector<double> wx = {-145.1165, -158.3417, -164.3164, -169.3365, -175.4917, -176.9617};
    const std::vector<double> wy = {4.339378, -17.42898, -30.18062, -42.84062, -66.52898, -76.85062};
    std::vector<std::vector<double>> poses;              // x, y, psi, v, steering, acceleration of every message
    std::vector<double> pose = {-146.7283, 1.660802, 4.125825, 26.6806, 0, 0};
    for (int warm = 0; warm < 2; warm++) {
      mpc.setWarmStart(warm != 0);
      if (mpc.getWarmStart() != (warm != 0)) return 1;
      long total = 0;
      for (int i = 0; i < steps; i++) {
        if (!warm) poses.push_back(pose);
        const std::vector<double> &p = poses[(size_t)i];
        Vehicle vehicle;
        vehicle.setLength(Config::Lf);
        vehicle.update(p[0], p[1], p[2], p[3], p[4], p[5]);
        std::vector<double> ptsx = wx, ptsy = wy;
        std::vector<double> v = mpc.run(vehicle, ptsx, ptsy);
        printf("%s %d %d %.12g %.12g %.12g %.12g %.12g %.12g %.12g %.12g\n", warm ? "warm" : "cold", i, mpc.lastIterations(), v[0], v[1], v[2], v[3],
               v[4], v[5], v[6], v[7]);
        total += mpc.lastIterations();
        if (!warm) {
          const double c = std::cos(p[2]), s = std::sin(p[2]);
          pose = {p[0] + v[0] * c - v[1] * s, p[1] + v[0] * s + v[1] * c, p[2] + v[2], v[3], v[4] * Config::maxSteering, v[5]};
        }
      }
      printf("%s total %ld\n", warm ? "warm" : "cold", total);
    }
  } catch (const std::string &e) {
    fprintf(stderr, "error: %s\n", e.c_str());
    return e.find("NO_DEVICE") != std::string::npos || e.find("no HIP device") != std::string::npos || e.find("mpc_create") != std::string::npos ? 3 : 1;
  }
  return 0;
}
