// Single-threaded host run of the connected-component algorithm of cswin_unet_amd/csrc/components.hip: the same find / union /
// link-rule code (components_uf.h) walked through the tile pass, the seam pass and the flatten pass in the kernels' order, against
// a flood fill.  It shows that the passes and the skipped links give the canonical labels and sizes, and that every loop ends,
// before any of it runs on a device.  Plain C++:
//   c++ -O1 -g -fsanitize=address,undefined -I cswin_unet_amd/csrc tools/components_host_check.cpp -o /tmp/cc_check && /tmp/cc_check
#include "components_uf.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

struct Vol {
    int D, H, W;
    std::vector<unsigned char> id;
    long n() const { return (long)D * H * W; }
    int at(int z, int y, int x) const { return id[((long)z * H + y) * W + x]; }
};

int fg(int b, int ncls) { return b < ncls ? b : 0; }

// labels / sizes the way the three launches produce them
void label_by_passes(const Vol& v, int ncls, std::vector<int>& labels, std::vector<int>& sizes) {
    const long N = v.n(), HW = (long)v.H * v.W;
    std::vector<int> parent(N, -1), tcnt(N, 0);
    const int nz = (v.D + CC_TZ - 1) / CC_TZ, ny = (v.H + CC_TY - 1) / CC_TY, nx = (v.W + CC_TX - 1) / CC_TX;
    auto idl = [&](int bz, int by, int bx, int l) {          // id of local voxel l of a tile, 0 outside the volume
        const int z = bz * CC_TZ + l / (CC_TY * CC_TX), y = by * CC_TY + (l / CC_TX) % CC_TY, x = bx * CC_TX + l % CC_TX;
        return (z < v.D && y < v.H && x < v.W) ? fg(v.at(z, y, x), ncls) : 0;
    };
    for (int bz = 0; bz < nz; ++bz)
        for (int by = 0; by < ny; ++by)
            for (int bx = 0; bx < nx; ++bx) {          // tile pass
                std::vector<int> lpar(CC_TILE_VOX), lcnt(CC_TILE_VOX, 0);
                const HostForest F = {lpar.data()};
                for (int l0 = 0; l0 < CC_TILE_VOX; l0 += CC_VOX) {
                    int run = l0;
                    for (int j = 0; j < CC_VOX; ++j) {
                        const int a = idl(bz, by, bx, l0 + j);
                        if (!(j > 0 && a != 0 && a == idl(bz, by, bx, l0 + j - 1))) run = l0 + j;
                        lpar[l0 + j] = run;
                    }
                }
                for (int l = 0; l < CC_TILE_VOX; ++l) {
                    const int lx = l % CC_TX, ly = (l / CC_TX) % CC_TY, lz = l / (CC_TY * CC_TX), a = idl(bz, by, bx, l);
                    const int am1 = lx > 0 ? idl(bz, by, bx, l - 1) : 0;
                    if (lx > 0 && lx % CC_VOX == 0 && a != 0 && am1 == a) cc_union(F, l, l - 1);
                    for (int axis = 0; axis < 2; ++axis) {
                        const int back = axis == 0 ? CC_TX : CC_TY * CC_TX;
                        if (axis == 0 ? ly == 0 : lz == 0) continue;
                        const int nb = idl(bz, by, bx, l - back), nbm1 = lx > 0 ? idl(bz, by, bx, l - back - 1) : 0;
                        if (cc_link_needed(a, nb, am1, nbm1)) cc_union(F, l, l - back);
                    }
                }
                for (int l = 0; l < CC_TILE_VOX; ++l) {
                    const int z = bz * CC_TZ + l / (CC_TY * CC_TX), y = by * CC_TY + (l / CC_TX) % CC_TY, x = bx * CC_TX + l % CC_TX;
                    if (!(z < v.D && y < v.H && x < v.W) || idl(bz, by, bx, l) == 0) continue;
                    const int r = cc_find(F, l);
                    ++lcnt[r];
                    const int rz = bz * CC_TZ + r / (CC_TY * CC_TX), ry = by * CC_TY + (r / CC_TX) % CC_TY, rx = bx * CC_TX + r % CC_TX;
                    parent[((long)z * v.H + y) * v.W + x] = (int)(((long)rz * v.H + ry) * v.W + rx);
                }
                for (int l = 0; l < CC_TILE_VOX; ++l)
                    if (lcnt[l]) {
                        const int z = bz * CC_TZ + l / (CC_TY * CC_TX), y = by * CC_TY + (l / CC_TX) % CC_TY, x = bx * CC_TX + l % CC_TX;
                        tcnt[((long)z * v.H + y) * v.W + x] = lcnt[l];
                    }
            }
    const HostForest G = {parent.data()};
    for (int z = 0; z < v.D; ++z)          // seam pass
        for (int y = 0; y < v.H; ++y)
            for (int x = 0; x < v.W; ++x) {
                const long i = ((long)z * v.H + y) * v.W + x;
                const int a = fg(v.at(z, y, x), ncls), lx = x % CC_TX, ly = y % CC_TY, lz = z % CC_TZ;
                const int am1 = lx > 0 ? fg(v.at(z, y, x - 1), ncls) : 0;
                if (ly == 0 && y > 0 && cc_link_needed(a, fg(v.at(z, y - 1, x), ncls), am1, lx > 0 ? fg(v.at(z, y - 1, x - 1), ncls) : 0))
                    cc_union(G, (int)i, (int)(i - v.W));
                if (lz == 0 && z > 0 && cc_link_needed(a, fg(v.at(z - 1, y, x), ncls), am1, lx > 0 ? fg(v.at(z - 1, y, x - 1), ncls) : 0))
                    cc_union(G, (int)i, (int)(i - HW));
                if (lx == 0 && x > 0 && cc_link_needed(a, fg(v.at(z, y, x - 1), ncls), ly > 0 ? fg(v.at(z, y - 1, x), ncls) : 0,
                                                       ly > 0 ? fg(v.at(z, y - 1, x - 1), ncls) : 0))
                    cc_union(G, (int)i, (int)(i - 1));
            }
    labels.assign(N, 0);
    sizes.assign(N, 0);
    for (long i = 0; i < N; ++i) {          // flatten pass
        if (parent[i] < 0) continue;
        const int r = cc_find(G, parent[i]);
        labels[i] = r + 1;
        if (tcnt[i] > 0) sizes[r] += tcnt[i];
    }
    for (long i = 0; i < N; ++i)
        if (parent[i] > i) {
            printf("parent[%ld] = %d breaks parent <= index\n", i, parent[i]);
            exit(1);
        }
}

void label_by_fill(const Vol& v, int ncls, std::vector<int>& labels, std::vector<int>& sizes) {
    const long N = v.n();
    labels.assign(N, 0);
    sizes.assign(N, 0);
    std::vector<long> stack;
    for (long s = 0; s < N; ++s) {
        const int a = fg(v.id[s], ncls);
        if (a == 0 || labels[s]) continue;
        labels[s] = (int)s + 1;
        stack.push_back(s);
        while (!stack.empty()) {
            const long i = stack.back();
            stack.pop_back();
            ++sizes[s];
            const int x = (int)(i % v.W), y = (int)((i / v.W) % v.H), z = (int)(i / ((long)v.H * v.W));
            const long nbr[6] = {x > 0 ? i - 1 : -1, x < v.W - 1 ? i + 1 : -1, y > 0 ? i - v.W : -1, y < v.H - 1 ? i + v.W : -1,
                                 z > 0 ? i - (long)v.H * v.W : -1, z < v.D - 1 ? i + (long)v.H * v.W : -1};
            for (long k : nbr)
                if (k >= 0 && !labels[k] && fg(v.id[k], ncls) == a) {
                    labels[k] = (int)s + 1;
                    stack.push_back(k);
                }
        }
    }
}

int failures = 0;
void check(const char* name, const Vol& v, int ncls) {
    std::vector<int> la, sa, lb, sb;
    label_by_passes(v, ncls, la, sa);
    label_by_fill(v, ncls, lb, sb);
    const bool ok = la == lb && sa == sb;
    printf("%-28s %4d x %4d x %4d  %s\n", name, v.D, v.H, v.W, ok ? "ok" : "MISMATCH");
    failures += !ok;
}

Vol make(int D, int H, int W, int fill = 0) { return Vol{D, H, W, std::vector<unsigned char>((size_t)D * H * W, (unsigned char)fill)}; }

Vol noise(int D, int H, int W, int ncls, double density, unsigned seed) {
    Vol v = make(D, H, W);
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    for (auto& b : v.id) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const double u = (double)(s >> 11) / 9007199254740992.0;
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        b = u < density ? (unsigned char)(1 + (s >> 33) % (ncls + 1)) : 0;          // ids up to ncls: one of them is out of range
    }
    return v;
}

// one class-1 path through every row of every layer, turning at alternate ends (rows and layers are joined by one voxel)
Vol serpentine(int D, int H, int W) {
    Vol v = make(D, H, W);
    for (int z = 0; z < D; z += 2) {
        for (int y = 0; y < H; y += 2) {
            for (int x = 0; x < W; ++x) v.id[((long)z * H + y) * W + x] = 1;
            if (y + 1 < H) v.id[((long)z * H + y + 1) * W + (((y / 2) % 2 == 0) ? W - 1 : 0)] = 1;
        }
        if (z + 1 < D) v.id[(long)(z + 1) * H * W] = 1;
    }
    return v;
}

// two tiles along `axis` (0 = z, 1 = y, 2 = x) and lanes across the seam between them: class 1 behind blocks of the ids a and b
// (both >= ncls) that face each other, class 1 facing such an id either way round, and one legal link as the control
Vol seam_lanes(int axis, int a, int b) {
    const int lanes[5][4] = {{1, a, b, 1}, {1, a, a, 1}, {0, 1, a, 0}, {0, a, 1, 0}, {2, 1, 1, 2}};
    const int T[3] = {CC_TZ, CC_TY, CC_TX}, t = T[axis], half = t / 2;
    int dim[3], k = 0;
    for (int d = 0; d < 3; ++d) dim[d] = d == axis ? 2 * t : (k++ == 0 ? 21 : 5);
    Vol v = make(dim[0], dim[1], dim[2]);
    for (int lane = 0; lane < 5; ++lane)
        for (int q = 0; q < 4; ++q)
            for (int s = q * half; s < (q + 1) * half; ++s)
                for (int u = 4 * lane + 1; u < 4 * lane + 4; ++u)
                    for (int w = 1; w < 4; ++w) {
                        int c[3], m = 0;
                        for (int d = 0; d < 3; ++d) c[d] = d == axis ? s : (m++ == 0 ? u : w);
                        v.id[((long)c[0] * v.H + c[1]) * v.W + c[2]] = (unsigned char)lanes[lane][q];
                    }
    return v;
}

}  // namespace

int main() {
    const int Z = CC_TZ, Y = CC_TY, X = CC_TX;
    check("noise small", noise(5, 9, 11, 4, 0.55, 1), 4);
    check("noise ragged tiles", noise(2 * Z + 1, 2 * Y + 3, 2 * X + 5, 4, 0.55, 2), 4);
    check("noise dense", noise(2 * Z + 1, Y + 3, X + 17, 2, 0.9, 3), 2);
    check("serpentine slice", serpentine(1, 4 * Y + 1, 4 * X + 2), 2);
    check("serpentine layers", serpentine(2 * Z + 1, Y + 1, X + 1), 2);
    {
        Vol v = make(Z + 1, Y + 2, X + 3);
        for (int z = 0; z < v.D; ++z)
            for (int y = 0; y < v.H; ++y)
                for (int x = 0; x < v.W; ++x) v.id[((long)z * v.H + y) * v.W + x] = (unsigned char)(1 + ((x + y + z) & 1));
        check("checkerboard", v, 3);
    }
    check("solid", make(Z + 1, 2 * Y, 2 * X + 1, 1), 2);
    check("solid, class out of range", make(Z + 1, Y, X, 5), 4);
    check("one voxel", make(1, 1, 1, 1), 2);
    check("row", make(1, 1, 3 * X + 7, 1), 2);
    check("column", make(1, 3 * Y + 5, 1, 1), 2);
    check("pillar", make(3 * Z + 2, 1, 1, 1), 2);
    // both ids above the site-percolation threshold (0.36 each): a spanning component per class among thousands of small ones.
    // ~10^5 voxels: there is no path compression, and one thread makes the chains as deep as they get
    check("noise percolating", noise(2 * Z + 1, 3 * Y + 2, 3 * X + 18, 1, 0.72, 4), 3);
    check("noise W % 4 == 2", noise(Z + 1, Y + 3, X + 2, 2, 0.8, 5), 3);
    for (int axis = 0; axis < 3; ++axis) {
        check("ids at and past ncls", seam_lanes(axis, 3, 200), 3);
        check("one id past ncls", seam_lanes(axis, 255, 255), 3);
    }
    if (failures) printf("%d case(s) FAILED\n", failures);
    else printf("all cases agree with the flood fill\n");
    return failures != 0;
}
