// clearance_host.cpp — the gaps and the motion radii of edmp_amd/csrc/clearance.h on the CPU, by a plain C++ compiler (built by
// __graft_entry__.build() with -ffp-contract=off; tests/test_certify_host.py holds the output to the rule of tests/certify_inputs.py).
//
// stdin: records, each a word followed by numbers (any form scanf's %la reads, hexadecimal floats included):
//   radii  28 numbers dh (7 x 4: a, d, cos(alpha), sin(alpha)), 108 numbers static frames (9 x 12, row-major 3 x 4), 27 half extents (9 x 3)
//   box    9 numbers R of the link box (row-major, columns = axes), 3 centre, 3 half extents, then the obstacle's 9 R, 3 centre, 3 half extents
//   cyl    the same numbers, the obstacle row read as a cylinder ((r, r, h) extents, halved)
// stdout, every number as %a: "rho" and 63 numbers (9 x 7) per radii record, "gap" and one number per box / cyl record.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "clearance.h"

static bool read_numbers(double* v, int n) {
    for (int i = 0; i < n; ++i)
        if (std::scanf("%la", &v[i]) != 1) return false;
    return true;
}

int main() {
    char word[16];
    while (std::scanf("%15s", word) == 1) {
        if (!std::strcmp(word, "radii")) {
            double dh[7][4], sf[9][12], he[9][3], rho[63];
            if (!read_numbers(&dh[0][0], 28) || !read_numbers(&sf[0][0], 108) || !read_numbers(&he[0][0], 27)) {
                std::fprintf(stderr, "clearance_host: a radii record holds 163 numbers\n");
                return 2;
            }
            edmp::motion_radii(dh, sf, he, rho);
            std::printf("rho");
            for (int i = 0; i < 63; ++i) std::printf(" %a", rho[i]);
            std::printf("\n");
        } else if (!std::strcmp(word, "box") || !std::strcmp(word, "cyl")) {
            double R[3][3], c[3], h[3], ob[16] = {0};
            if (!read_numbers(&R[0][0], 9) || !read_numbers(c, 3) || !read_numbers(h, 3) || !read_numbers(ob, 15)) {
                std::fprintf(stderr, "clearance_host: a %s record holds 30 numbers\n", word);
                return 2;
            }
            std::printf("gap %a\n", word[0] == 'b' ? edmp::box_box_gap(R, c, h, ob) : edmp::box_cylinder_gap(R, c, h, ob));
        } else {
            std::fprintf(stderr, "clearance_host: unknown record '%s'\n", word);
            return 2;
        }
    }
    return 0;
}
