// The builders' compact 80-B node as the 64-B node (bvh_build.h): the
// non-empty slots become children 0..5 in slot order, the group word is the
// first inner child.  Shared by refit_check.cpp and bvh_dump.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

// *over is set when a node has more than six children (the tree is not width 6).
inline std::vector<uint32_t> to_node6(const std::vector<uint32_t>& n8, bool* over) {
    const size_t nn = n8.size() / 20;
    std::vector<uint32_t> out(nn * 16, 0u);
    *over = false;
    for (size_t i = 0; i < nn; i++) {
        const uint32_t* w = &n8[i * 20];
        uint32_t meta[6] = {0, 0, 0, 0, 0, 0}, q[6][6];
        for (int p = 0; p < 6; p++)
            for (int c = 0; c < 6; c++) q[p][c] = (p & 1) ? 0u : 255u;
        int c = 0;
        for (uint32_t s = 0; s < 8; s++) {
            const uint32_t sh = (s & 3u) * 8u, m = (w[6 + (s >> 2)] >> sh) & 0xffu;
            if (!m) continue;
            if (c == 6) { *over = true; break; }
            meta[c] = m;
            for (int a = 0; a < 3; a++) {
                q[2 * a][c] = (w[8 + 2 * a + (s >> 2)] >> sh) & 0xffu;
                q[2 * a + 1][c] = (w[14 + 2 * a + (s >> 2)] >> sh) & 0xffu;
            }
            c++;
        }
        uint32_t* o = &out[i * 16];
        o[0] = w[0]; o[1] = w[1]; o[2] = w[2]; o[3] = w[5];
        o[4] = meta[0] | meta[1] << 8 | meta[2] << 16 | meta[3] << 24;
        o[5] = meta[4] | meta[5] << 8 | (w[3] & 0xffu) << 16 | ((w[3] >> 8) & 0xffu) << 24;
        o[6] = w[4] | ((w[3] >> 16) & 0xffu) << 24;
        for (int p = 0; p < 6; p++) o[7 + p] = q[p][0] | q[p][1] << 8 | q[p][2] << 16 | q[p][3] << 24;
        for (int a = 0; a < 3; a++)
            o[13 + a] = q[2 * a][4] | q[2 * a][5] << 8 | q[2 * a + 1][4] << 16 | q[2 * a + 1][5] << 24;
    }
    return out;
}
