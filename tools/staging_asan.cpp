// Staging's reservation arithmetic (offsets, alignment, totals, growth) under
// ASan + UBSan: csrc/mvs_host.h compiled as host C++ against stubbed HIP calls
// (malloc / memcpy); no GPU, no GPU runtime linked.  From the package's csrc/:
//   /opt/rocm/lib/llvm/bin/clang++ -x c++ -std=c++17 -O1 -g -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I. \
//     -fsanitize=address,undefined -fno-sanitize-recover=undefined ../../tools/staging_asan.cpp -o /tmp/staging_asan
//   /tmp/staging_asan        (log: profiles/r15/staging_asan.log)
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mvs_host.h"

static size_t g_mallocs = 0;
extern "C" {
hipError_t hipMalloc(void** p, size_t n) { *p = std::malloc(n); ++g_mallocs; return *p ? hipSuccess : hipErrorOutOfMemory; }
hipError_t hipFree(void* p) { std::free(p); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { std::memcpy(d, s, n); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
}

template <class T>
static void fill(std::vector<T>& v, unsigned seed) {
    for (size_t i = 0; i < v.size(); ++i) v[i] = (T)(seed * 2654435761u + i * 40503u);
}

// one call with arrays of four element sizes: every byte in comes back out through a device-side copy
static void round_trip(Staging& st, size_t n, bool optional) {
    const size_t m1 = n ? n : 1;      // a host array is never null here, also at n = 0
    std::vector<double> a(3 * m1), a2(3 * m1);
    std::vector<int32_t> b(m1), b2(m1);
    std::vector<uint8_t> c(m1), c2(m1);
    std::vector<int4> j(m1);
    fill(a, 1); fill(b, 2); fill(c, 3);
    for (size_t i = 0; i < n; ++i) j[i] = int4{(int)i, 1, 2, 3};
    st.begin(nullptr);
    const auto da = st.in(a.data(), 3 * n);
    const auto db = st.in(b.data(), n);
    const auto dc = st.in(c.data(), n);
    const auto dj = st.in(j.data(), n);
    const auto dnull = st.in((const double*)nullptr, n);          // reserved, not copied
    const auto oa = st.out(a2.data(), 3 * n);
    const auto ob = st.out(b2.data(), n);
    const auto oc = st.out(c2.data(), n);
    const auto oopt = st.out(optional ? a2.data() : (double*)nullptr, 0);
    const auto onull = st.out((double*)nullptr, n);
    const auto tmp = st.tmp<uint64_t>(n);
    bool threw = false;
    try { (void)(double*)da; } catch (const Fail&) { threw = true; }
    assert(threw);                                                  // no pointer before upload
    const size_t mallocs = g_mallocs, cap = st.buf.n;
    st.upload();
    assert(st.buf.n >= st.total && (st.total <= cap ? g_mallocs == mallocs && st.buf.n == cap
                                                    : g_mallocs == mallocs + 1 && st.buf.n == std::max(st.total, 2 * cap)));
    threw = false;
    try { st.tmp<int>(1); } catch (const Fail&) { threw = true; }
    assert(threw);                                                  // no slot after upload
    unsigned char* lo = st.buf.p;
    unsigned char* hi = st.buf.p + st.buf.n;
    const void* ps[] = {(double*)da, (int32_t*)db, (uint8_t*)dc, (int4*)dj, (double*)dnull, (double*)oa, (int32_t*)ob,
                        (uint8_t*)oc, (uint64_t*)tmp};
    const size_t bytes[] = {24 * n, 4 * n, n, 16 * n, 8 * n, 24 * n, 4 * n, n, 8 * n};
    for (int k = 0; k < 9; ++k) {
        const unsigned char* p = (const unsigned char*)ps[k];
        assert(p >= lo && p + bytes[k] <= hi && ((p - lo) % Staging::kAlign) == 0);
        for (int m = 0; m < k; ++m) {                               // slots do not overlap
            const unsigned char* q = (const unsigned char*)ps[m];
            assert(n == 0 || p + bytes[k] <= q || q + bytes[m] <= p);
        }
    }
    assert((double*)onull == nullptr);
    assert(optional ? (double*)oopt != nullptr : (double*)oopt == nullptr);
    if (n) {
        std::memcpy((double*)oa, (double*)da, 24 * n);
        std::memcpy((int32_t*)ob, (int32_t*)db, 4 * n);
        std::memcpy((uint8_t*)oc, (uint8_t*)dc, n);
        std::memset((uint64_t*)tmp, 0xab, 8 * n);
        assert(((int4*)dj)[n - 1].x == (int)n - 1);
    }
    st.finish();
    assert(n == 0 || (a == a2 && b == b2 && c == c2));
}

int main() {
    Staging st;
    const size_t sizes[] = {257, 300, 5, 0, 1, 3, 4099, 4, 7, 70000, 1};
    for (size_t n : sizes) {
        round_trip(st, n, n % 2 == 1);
        std::printf("n %zu: total %zu B, arena %zu B, %zu allocations\n", n, st.total, st.buf.n, g_mallocs);
    }
    return 0;
}
