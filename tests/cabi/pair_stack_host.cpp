// Host build of polytope_amd/csrc/plp_pair_stack.hpp (the stack rule of plp_pair_stacks / plp_intersect_pairs and its
// sequential restatement): TEST INFRASTRUCTURE, compiled with g++ -ffp-contract=off by tests/pair_stack_host.py.  The device
// kernel of plp_pair_stack.hip is held against these functions, bit for bit.
//
// -DPAIR_STACK_HOST_MAIN adds a main(): a stand-alone program that reads tables, pair lists and the stacks to expect from a
// binary file (written by the test from its own run) and forms the stacks again, for a run under
// -fsanitize=address,undefined without anything loaded into an interpreter.
#include <stdint.h>

#include "../../polytope_amd/csrc/plp_pair_stack.hpp"

extern "C" {

// the first bad pair of the list, or -1
long long psh_first_bad(int n, long long K, const int32_t* pairs) { return plp::ps::host_first_bad(n, K, pairs); }

// 0; 1: a bad pair in the list (nothing written); 2: sizes outside 2 m_max <= 64, d <= 16
int psh_stacks(int n, int m_max, int d, const double* A, const double* b, const int32_t* m, long long K, const int32_t* pairs,
               double* A_s, double* b_s, int32_t* m_s) {
    if (plp::ps::host_first_bad(n, K, pairs) >= 0) return 1;
    return plp::ps::host_stacks(n, m_max, d, A, b, m, K, pairs, A_s, b_s, m_s);
}

// as psh_stacks without the check of the list: a bad pair gets m_s = 0 and zero rows, as on the device
int psh_stacks_unchecked(int n, int m_max, int d, const double* A, const double* b, const int32_t* m, long long K,
                         const int32_t* pairs, double* A_s, double* b_s, int32_t* m_s) {
    return plp::ps::host_stacks(n, m_max, d, A, b, m, K, pairs, A_s, b_s, m_s);
}

}  // extern "C"

#ifdef PAIR_STACK_HOST_MAIN
#include <stdio.h>
#include <string.h>

#include <vector>

// file: int64 n_cases; per case int64 n, m_max, d, K; then A[n m_max d], b[n m_max] (float64), m[n], pairs[2 K] (int32),
// and the expected A_s[K 2m_max d], b_s[K 2m_max] (float64), m_s[K] (int32).  Every array is read into an allocation of
// exactly its size, so that a read or write past an end is the sanitizer's to find.
template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t n_cases = 0;
    if (fread(&n_cases, 8, 1, f) != 1) return 2;
    long long checked = 0;
    for (int64_t c = 0; c < n_cases; ++c) {
        int64_t hd[4];
        if (fread(hd, 8, 4, f) != 4) return 2;
        const int n = (int)hd[0], m_max = (int)hd[1], d = (int)hd[2];
        const long long K = hd[3];
        const size_t W = 2 * (size_t)m_max;
        std::vector<double> A, b, As, bs;
        std::vector<int32_t> m, pairs, ms;
        if (!rd(f, A, (size_t)n * m_max * d) || !rd(f, b, (size_t)n * m_max) || !rd(f, m, (size_t)n) ||
            !rd(f, pairs, (size_t)K * 2) || !rd(f, As, (size_t)K * W * d) || !rd(f, bs, (size_t)K * W) || !rd(f, ms, (size_t)K))
            return 2;
        std::vector<double> A2((size_t)K * W * d, -7.0), b2((size_t)K * W, -7.0);
        std::vector<int32_t> m2((size_t)K, -7);
        const int rc = psh_stacks(n, m_max, d, A.data(), b.data(), m.data(), K, pairs.data(), A2.data(), b2.data(), m2.data());
        if (rc != 0) {
            fprintf(stderr, "case %lld: psh_stacks returned %d\n", (long long)c, rc);
            return 1;
        }
        if ((A2.size() && memcmp(A2.data(), As.data(), A2.size() * 8)) || (b2.size() && memcmp(b2.data(), bs.data(), b2.size() * 8)) ||
            (m2.size() && memcmp(m2.data(), ms.data(), m2.size() * 4))) {
            fprintf(stderr, "case %lld: the stacks differ from the recorded ones\n", (long long)c);
            return 1;
        }
        checked += K;
    }
    fclose(f);
    printf("pair_stack_host: %lld cases, %lld stacks, all equal\n", (long long)n_cases, checked);
    return 0;
}
#endif
