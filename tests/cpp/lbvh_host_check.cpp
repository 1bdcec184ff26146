// lbvh_host_check — the integer core of the device BVH build (rrte_amd/csrc/mesh_build.hpp) on the
// host, for tests/test_lbvh_cpu.py, which builds it with -fsanitize=address,undefined.  Runs exactly
// the __host__ __device__ functions the kernels call.  Commands on stdin, one per line:
//   K n k0 .. k(n-1)   the radix tree over n ascending unique 64-bit leaf keys.  Prints "tree n", then
//                      per record "rec i c0 c1 axis parent depth first last" (a child that is leaf j
//                      prints as -(j + 1), a record as its index; parent is a code record * 2 + side
//                      or -1) and per leaf "leaf j parent".
//   M qx qy qz         prints "morton code".
//   C c lo ext         (three f32 bit patterns, decimal) prints "cell q".
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../rrte_amd/csrc/mesh_build.hpp"

using namespace rrte;

static float bits_f(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "M") {
            uint32_t q[3];
            if (!(in >> q[0] >> q[1] >> q[2])) return 2;
            std::printf("morton %u\n", lbvh_morton(q[0], q[1], q[2]));
        } else if (cmd == "C") {
            uint32_t b[3];
            if (!(in >> b[0] >> b[1] >> b[2])) return 2;
            std::printf("cell %u\n", lbvh_cell(bits_f(b[0]), bits_f(b[1]), bits_f(b[2])));
        } else if (cmd == "K") {
            size_t n = 0;
            if (!(in >> n)) return 2;
            std::vector<uint64_t> keys(n);
            for (uint64_t& k : keys)
                if (!(in >> k)) return 2;
            std::printf("tree %zu\n", n);
            if (n < 2) continue;
            const uint32_t recs = (uint32_t)n - 1u;
            std::vector<uint32_t> parent(recs, kLbvhNoParent), leaf_parent(n, kLbvhNoParent), axis(recs);
            std::vector<LbvhNode> nodes(recs);
            std::vector<long long> child(2 * (size_t)recs);
            for (uint32_t i = 0; i < recs; ++i) {
                const LbvhNode nd = nodes[i] = lbvh_node(keys.data(), (uint32_t)n, i);
                if (nd.last >= n || nd.split >= nd.last || nd.first > nd.split) return 3;
                for (uint32_t side = 0; side < 2; ++side) {
                    const uint32_t a = side ? nd.split + 1 : nd.first, b = side ? nd.last : nd.split;
                    if (a == b) {
                        child[2 * (size_t)i + side] = -(long long)a - 1;
                        leaf_parent[a] = i * 2 + side;
                    } else {
                        const uint32_t c = side ? nd.split + 1 : nd.split;
                        if (c >= recs) return 3;
                        child[2 * (size_t)i + side] = c;
                        parent[c] = i * 2 + side;
                    }
                }
                axis[i] = lbvh_axis(keys[nd.split], keys[nd.split + 1]);
            }
            for (uint32_t i = 0; i < recs; ++i)
                std::printf("rec %u %lld %lld %u %lld %u %u %u\n", i, child[2 * (size_t)i], child[2 * (size_t)i + 1], axis[i],
                            parent[i] == kLbvhNoParent ? -1ll : (long long)parent[i], lbvh_depth(parent.data(), i),
                            nodes[i].first, nodes[i].last);
            for (size_t j = 0; j < n; ++j)
                std::printf("leaf %zu %lld\n", j, leaf_parent[j] == kLbvhNoParent ? -1ll : (long long)leaf_parent[j]);
        } else {
            return 2;
        }
    }
    return 0;
}
