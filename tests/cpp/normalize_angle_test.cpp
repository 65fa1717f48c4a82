/* normalizeAngle of include/mpc_drop_in.hpp beside mpc::normalize_angle of csrc/mpc_run_core.h (its host build), host code only:
 * every argument a double in hexadecimal notation (or inf / nan); one line per argument with both results, as printf's %a. */
#include <cstdio>
#include <cstdlib>

#include "mpc_drop_in.hpp"
#include "mpc_run_core.h"

int main(int argc, char **argv) {
  for (int i = 1; i < argc; i++) {
    const double a = strtod(argv[i], nullptr);
    printf("%a %a %a\n", a, normalizeAngle(a), mpc::normalize_angle(a));
  }
  return 0;
}
