// Test helper (tests/test_controller.py): the product's own ctl::clamp_angle, host side, over an array.
// Reads raw doubles from stdin, writes clamp_angle of each to stdout, same format.  The caller runs it under a timeout.
#include <cstdio>

#include "../../armour_amd/csrc/controller_core.h"

int main() {
    double x;
    while (fread(&x, sizeof x, 1, stdin) == 1) {
        const double r = ctl::clamp_angle(x);
        if (fwrite(&r, sizeof r, 1, stdout) != 1) return 1;
    }
    return fflush(stdout) == 0 ? 0 : 1;
}
