// launch_grids.cpp -- obia_test_launch_grid / obia_test_launch_grid_names (include/obia_testing.h): the named grids of launch_grids.hpp
// for the test suite.  Pure host code: no context, nothing is launched.
#include <cstring>
#include <string>

#include "common.hpp"

using namespace obia;

extern "C" int obia_test_launch_grid(const char *name, const int64_t *sizes, int n_sizes, int64_t *out4) {
    if (!name || !sizes || !out4) { set_error("obia_test_launch_grid: bad arguments"); return OBIA_E_INVALID; }
    int count = 0;
    const grids::Named *t = grids::table(&count);
    for (int i = 0; i < count; ++i) {
        if (strcmp(t[i].name, name) != 0) continue;
        if (n_sizes != t[i].n_sizes) {
            set_error("obia_test_launch_grid: `%s` takes %d sizes (%s), got %d", name, t[i].n_sizes, t[i].sizes, n_sizes);
            return OBIA_E_INVALID;
        }
        long long s[4] = {0, 0, 0, 0};
        for (int k = 0; k < n_sizes; ++k) {
            if (sizes[k] < 1 || sizes[k] > grids::GRID_X_MAX) {
                set_error("obia_test_launch_grid: `%s`: size %d must be in 1 .. 2^31 - 1, got %lld", name, k, (long long)sizes[k]);
                return OBIA_E_INVALID;
            }
            s[k] = sizes[k];
        }
        const grids::Grid g = t[i].fn(s);
        out4[0] = g.x.n; out4[1] = g.y.n; out4[2] = g.x.trips; out4[3] = g.y.trips;
        return OBIA_OK;
    }
    set_error("obia_test_launch_grid: no launch is named `%s`", name);
    return OBIA_E_INVALID;
}

extern "C" int obia_test_launch_grid_names(char *text, int64_t text_bytes) {
    if (!text || text_bytes < 1) { set_error("obia_test_launch_grid_names: bad arguments"); return OBIA_E_INVALID; }
    int count = 0;
    const grids::Named *t = grids::table(&count);
    std::string s;
    for (int i = 0; i < count; ++i) s += std::string(t[i].name) + " " + t[i].sizes + "\n";
    if ((int64_t)s.size() + 1 > text_bytes) { set_error("obia_test_launch_grid_names: the text needs %zu bytes", s.size() + 1); return OBIA_E_INVALID; }
    memcpy(text, s.c_str(), s.size() + 1);
    return OBIA_OK;
}
