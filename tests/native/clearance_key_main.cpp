// A stand-alone check of clearanceKey (csrc/clearance.hpp), the order-preserving 64-bit key the batch's integer atomicMin reduces:
//   key(x) < key(y) iff x < y and key(x) == key(y) iff x == y        over +-0, +-subnormals, +-DBL_MAX, +inf, -inf and random doubles;
//   clearanceKeyValue(key(x)) == x, with +0.0 for either zero;
//   the minimum the batch takes -- the least key, then the least pos among its holders -- is clearanceBefore's, +-0 ties included.
// No device and no library:
//   g++ -std=c++17 -O1 -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Icsrc -Iinclude tests/native/clearance_key_main.cpp
// (csrc = hp-adaptive-signed-distance-field-octree_amd/csrc).  Exit status 0 and a last line "OK <pairs compared>".
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "clearance.hpp"

int main() {
    using namespace hpsdf;
    std::vector<double> v;
    const double inf = boundsInf();
    for (double s : {1.0, -1.0}) {
        v.push_back(s * 0.0), v.push_back(s * DBL_TRUE_MIN), v.push_back(s * 3 * DBL_TRUE_MIN), v.push_back(s * DBL_MIN);
        v.push_back(s * (DBL_MIN - DBL_TRUE_MIN)), v.push_back(s * DBL_MAX), v.push_back(s * inf), v.push_back(s * 1.0), v.push_back(s * 0.75);
    }
    std::mt19937_64 gen(1601);
    while (v.size() < 3000) {  // random bit patterns (every exponent) and random values near one another
        const uint64_t u = gen();
        double x;
        std::memcpy(&x, &u, sizeof x);
        if (x == x) v.push_back(x);
        v.push_back(1.0 + (double)(gen() % 64) * DBL_EPSILON);
        v.push_back(-1e-300 * (double)(gen() % 16));
    }
    long bad = 0, pairs = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        const double back = clearanceKeyValue(clearanceKey(v[i]));
        if (!(back == v[i]) || (v[i] != 0.0 && std::memcmp(&back, &v[i], sizeof back) != 0) || (v[i] == 0.0 && std::signbit(back))) ++bad;
        if (!(clearanceKey(v[i]) < kClearanceNoKey)) ++bad;
        for (size_t j = 0; j < v.size(); ++j, ++pairs) {
            const uint64_t a = clearanceKey(v[i]), b = clearanceKey(v[j]);
            if ((a < b) != (v[i] < v[j]) || (a == b) != (v[i] == v[j])) ++bad;
        }
    }
    if (clearanceKeyValue(kClearanceNoKey) != inf) ++bad;
    // the two-step minimum against clearanceBefore over short lists with many ties (values from a small set that holds both zeros)
    const double few[] = {-0.0, 0.0, -1.5, 2.0, DBL_TRUE_MIN, -DBL_TRUE_MIN};
    for (int round = 0; round < 20000; ++round) {
        const uint32_t n = 1u + (uint32_t)(gen() % 9);
        double x[9];
        for (uint32_t i = 0; i < n; ++i) x[i] = few[gen() % 6];
        ClearanceCandidate c{inf, 0.0, kClearanceNoPos};
        for (uint32_t i = 0; i < n; ++i)
            if (clearanceBefore(x[i], i, c.vb, c.pos)) c.vb = x[i], c.pos = i;
        uint64_t key = kClearanceNoKey;
        for (uint32_t i = n; i-- > 0;) key = clearanceKey(x[i]) < key ? clearanceKey(x[i]) : key;  // (any order)
        uint32_t pos = kClearanceNoPos;
        for (uint32_t i = n; i-- > 0;)
            if (clearanceKey(x[i]) == key && i < pos) pos = i;
        if (pos != c.pos || std::memcmp(&x[pos], &c.vb, sizeof(double)) != 0) ++bad;
    }
    if (bad) {
        std::printf("%ld checks failed\n", bad);
        return 1;
    }
    std::printf("OK %ld\n", pairs);
    return 0;
}
