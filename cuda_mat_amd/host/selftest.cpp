// selftest.cpp -- host-only checks that run under AddressSanitizer (make -C cuda_mat_amd/host asan-check):
// the Matrix Market loader on the shipped fixtures and on hostile files, toDenseVector, Matrix.h, and the owner type
// of device memory (csrc/owned.h) on malloc'ed blocks.
// No GPU is touched: sanitizers are for the CPU side (the pool has no GPU AddressSanitizer).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "Matrix.h"
#include "cudamat.h"
#include "owned.h"

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static std::string write_file(const std::string &dir, const char *name, const char *text)
{
    const std::string path = dir + "/" + name;
    FILE *f = std::fopen(path.c_str(), "w");
    if (f) { std::fputs(text, f); std::fclose(f); }
    return path;
}

static int load(const std::string &path, bool csr, int *m, int *n, int *nnz, double **v, int **r, int **c)
{
    return cudamat_load_mtx(path.c_str(), csr ? 1 : 0, m, n, nnz, v, r, c);
}

// ---- csrc/owned.h: every block is freed exactly once (the sanitizer sees a double free; its leak check at exit a missing one)
static int frees = 0;
static void counting_free(void *p)
{
    frees++;
    std::free(p);
}
using IntBuf = cm::Owned<int, counting_free>;
static int *block() { return (int *)std::malloc(4 * sizeof(int)); }

static void check_owned()
{
    frees = 0;
    {
        IntBuf a;                                  // empty: nothing to free
        EXPECT(a.get() == nullptr && !a);
    }
    EXPECT(frees == 0);
    {
        IntBuf a;
        a.adopt(block());
        EXPECT(a.get() != nullptr);
        int *raw = a;                              // implicit conversion, pointer arithmetic
        EXPECT(raw == a.get() && a + 1 == raw + 1);
    }
    EXPECT(frees == 1);                            // the destructor frees once
    {
        IntBuf a;
        a.adopt(block());
        int *p = a.get();
        IntBuf b(std::move(a));
        EXPECT(a.get() == nullptr && b.get() == p);
    }
    EXPECT(frees == 2);                            // a moved-from owner frees nothing
    {
        IntBuf a, b;
        a.adopt(block());
        b.adopt(block());
        int *pb = b.get();
        a = std::move(b);
        EXPECT(frees == 3);                        // move assignment frees the old block, once and at that point
        EXPECT(a.get() == pb && b.get() == nullptr);
        IntBuf &self = a;
        a = std::move(self);
        EXPECT(frees == 3 && a.get() == pb);       // self-move keeps the block
        a.adopt(a.get());
        EXPECT(frees == 3 && a.get() == pb);       // adopting its own pointer is a no-op
        a.adopt(block());
        EXPECT(frees == 4 && a.get() != pb);       // adopting another frees what it held
    }
    EXPECT(frees == 5);
    {
        IntBuf a;
        a.adopt(block());
        int *p = a.release();                      // given up, not freed
        EXPECT(frees == 5 && a.get() == nullptr);
        std::free(p);
        a.adopt(block());
        a.reset();
        a.reset();
        EXPECT(frees == 6 && a.get() == nullptr);  // reset() twice frees once
    }
    EXPECT(frees == 6);
    {
        // the shape of the refactorisation's value maps (csrc/ilu.h, IluPlans::FactorSrc): one owner and a vector of owners
        // inside a struct that is resized, filled with gaps, rebuilt, and dropped by assigning an empty one
        struct Maps {
            IntBuf near;
            std::vector<IntBuf> far;
        } m;
        m.near.adopt(block());
        m.far.resize(5);                           // (groups without a far part stay empty)
        for (size_t g = 1; g < m.far.size(); g += 2) m.far[g].adopt(block());
        EXPECT(frees == 6 && !m.far[0] && m.far[1].get() != nullptr && m.far[3].get() != nullptr);
        m.far.clear();
        EXPECT(frees == 8);                        // clear() frees what the elements held
        m.far.resize(9);                           // (reallocation moves owners, it never copies or frees them)
        m.far[8].adopt(block());
        m.far.resize(64);
        EXPECT(frees == 8 && m.far[8].get() != nullptr);
        m = Maps();                                // a failed build leaves nothing half built
        EXPECT(frees == 10 && !m.near && m.far.empty());
        m.near.adopt(block());
    }
    EXPECT(frees == 11);
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: selftest <golden dir> <scratch dir>\n"); return 2; }
    const std::string gold = argv[1], tmp = argv[2];
    int m, n, nnz;
    double *v;
    int *r, *c;
    // shipped fixtures: sizes the reference's loader reports
    struct { const char *file; int n, nnz; } fixtures[] = {{"mat3.mtx", 3, 8}, {"mat900.mtx", 900, 7744}, {"mat10000.mtx", 10000, 49600}};
    for (auto &fx : fixtures) {
        for (int csr = 0; csr < 2; csr++) {
            v = nullptr; r = c = nullptr;
            EXPECT(load(gold + "/" + fx.file, csr, &m, &n, &nnz, &v, &r, &c) == CUDAMAT_OK);
            EXPECT(m == fx.n && n == fx.n && nnz == fx.nnz);
            if (v) {
                const int *ptr = csr ? r : c;
                EXPECT(ptr[0] == 1 && ptr[fx.n] == 1 + fx.nnz);
            }
            cudamat_host_free(v); cudamat_host_free(r); cudamat_host_free(c);
        }
    }
    // vec3_d: rows 1 and 3 only -> dense [1, 0, 1]
    v = nullptr; r = c = nullptr;
    EXPECT(load(gold + "/vec3_d.mtx", true, &m, &n, &nnz, &v, &r, &c) == CUDAMAT_OK);
    if (v) {
        double dense[3] = {-1, -1, -1};
        cudamat_to_dense_vector(m, nnz, v, r, dense);
        EXPECT(dense[0] == 1.0 && dense[1] == 0.0 && dense[2] == 1.0);
    }
    cudamat_host_free(v); cudamat_host_free(r); cudamat_host_free(c);
    // hostile files: every one must come back as an error, with nothing leaked or overrun
    const char *bad[][2] = {
        {"huge.mtx", "%%MatrixMarket matrix coordinate real general\n3 3 2147483647\n1 1 1\n"},
        {"hugesym.mtx", "%%MatrixMarket matrix coordinate real symmetric\n3 3 1500000000\n1 1 1\n"},
        {"widecol.mtx", "%%MatrixMarket matrix coordinate real general\n3 3 2\n1 1 1\n2 7 2\n"},
        {"widerow.mtx", "%%MatrixMarket matrix coordinate real general\n3 3 2\n1 1 1\n9 2 2\n"},
        {"dup.mtx", "%%MatrixMarket matrix coordinate real general\n3 3 3\n1 1 1\n1 1 2\n3 3 1\n"},
        {"short.mtx", "%%MatrixMarket matrix coordinate real general\n3 3 3\n1 1 1\n2 2 2\n"},
        {"both.mtx", "%%MatrixMarket matrix coordinate real general\n3 3 2\n0 1 1\n3 3 2\n"},
        {"empty.mtx", ""},
    };
    for (auto &b : bad) {
        v = nullptr; r = c = nullptr;
        EXPECT(load(write_file(tmp, b[0], b[1]), true, &m, &n, &nnz, &v, &r, &c) != CUDAMAT_OK);
    }
    EXPECT(load(tmp + "/does_not_exist.mtx", true, &m, &n, &nnz, &v, &r, &c) != CUDAMAT_OK);
    // symmetric expansion incl. skew sign, on a file written here
    v = nullptr; r = c = nullptr;
    EXPECT(load(write_file(tmp, "skew.mtx", "%%MatrixMarket matrix coordinate real skew-symmetric\n3 3 2\n2 1 5\n3 3 7\n"), true,
                &m, &n, &nnz, &v, &r, &c) == CUDAMAT_OK);
    EXPECT(nnz == 3);
    if (v && nnz == 3) EXPECT(v[0] == -5.0 && v[1] == 5.0 && v[2] == 7.0);
    cudamat_host_free(v); cudamat_host_free(r); cudamat_host_free(c);

    // Matrix.h
    Matrix<double> A(2, 3, {1, 2, 3, 4, 5, 6});
    Matrix<double> At = Matrix<double>::transpose(A);
    EXPECT(At.n == 3 && At.m == 2 && At.get(2, 0) == 3 && At.get(0, 1) == 4);
    Matrix<double> G = mul(A, At);                 // [[14, 32], [32, 77]]
    EXPECT(G.get(0, 0) == 14 && G.get(0, 1) == 32 && G.get(1, 1) == 77);
    EXPECT(mul(Matrix<double>::identity(2), A).get(1, 2) == 6);
    EXPECT(Matrix<double>::without_column(A, 1).get(1, 1) == 6 && A.column(2).get(1, 0) == 6 && A.row(1).get(0, 0) == 4);
    EXPECT(Matrix<double>::is_zero(Matrix<double>(2, 2, 0.0), 1e-12) && !Matrix<double>::is_zero(A, 1e-12));
    std::vector<double> val;
    std::vector<int> rp, ci;
    EXPECT(Matrix<double>(2, 2, {4, 0, -1, 4}).to_csr(1, &val, &rp, &ci) == 3 && rp[2] == 4 && ci[1] == 1);
    bool threw = false;
    try { A.get(2, 0); } catch (const std::out_of_range &) { threw = true; }
    EXPECT(threw);
    check_owned();
    if (failures == 0) std::printf("SELFTEST_OK\n");
    return failures ? 1 : 0;
}
