// Stand-alone check of pixray_amd/csrc/dev_arena.h (host code) against the hipemu runtime, meant for -fsanitize=address,undefined:
// `make -C tools/hipemu arena-check` builds and runs it.  A handle that owns a DevArena is created under a std::unique_ptr as the
// runners do; every one of its allocations is refused in turn through hipemu_fail_alloc; each time the create must return -1 with
// the figures in the message and leave nothing allocated, and a create that succeeds must free everything when it is deleted.
#include "dev_arena.h"
#include <memory>
#include <string.h>

extern "C" void hipemu_live_allocs(long long* count, long long* bytes);
extern "C" long long hipemu_fail_alloc(long long k);

static char g_err[512];
void prx_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {
struct Handle {
    int n = 0;
    DevArena mem;
    float* a = nullptr;
    void* b = nullptr;
    float* c = nullptr;
    double* d = nullptr;
};
constexpr int N_ALLOC = 4;

int create(Handle** out, int n, const float* src) {
    std::unique_ptr<Handle> guard(new Handle());
    Handle* h = guard.get();
    h->n = n;
    h->mem.describe("arena_check", ": the handle keeps %d elements", n);
    DEV_ALLOC(h->mem, alloc, h->a, (size_t)n);
    DEV_ALLOC(h->mem, alloc_op, h->b, (size_t)n, 0);
    if (int r = h->mem.copy_f32(&h->c, src, (size_t)n, 0)) return r;
    DEV_ALLOC(h->mem, alloc, h->d, 0);                          // a count of 0: one element
    *out = guard.release();
    return 0;
}
void live(long long* count, long long* bytes) { hipemu_live_allocs(count, bytes); }
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "arena_check: line %d: %s (last error: %s)\n", __LINE__, #cond, g_err); return 1; } } while (0)
}  // namespace

int main() {
    const int n = 1000;
    std::unique_ptr<float[]> src(new float[n]);
    for (int i = 0; i < n; ++i) src[i] = (float)i;
    long long c0, b0, c1, b1;
    live(&c0, &b0);
    const size_t held_before[N_ALLOC] = {0, (size_t)n * 4, (size_t)n * 6, (size_t)n * 10};
    for (int k = 0; k < N_ALLOC; ++k) {
        Handle* h = nullptr;
        hipemu_fail_alloc(k);
        const int rc = create(&h, n, src.get());
        const long long at_failure = hipemu_fail_alloc(-1);
        CHECK(rc == -1 && h == nullptr);
        char want[128];
        snprintf(want, sizeof(want), "with %zu bytes already held by this handle: the handle keeps %d elements", held_before[k], n);
        CHECK(strstr(g_err, "arena_check: device allocation of ") == g_err && strstr(g_err, want));
        CHECK((size_t)(at_failure - b0) == held_before[k]);
        live(&c1, &b1);
        CHECK(c1 == c0 && b1 == b0);
    }
    Handle* h = nullptr;
    CHECK(create(&h, n, src.get()) == 0 && h);
    live(&c1, &b1);
    CHECK(c1 - c0 == N_ALLOC && (size_t)(b1 - b0) == h->mem.bytes() && h->mem.bytes() == (size_t)n * 10 + sizeof(double));
    for (int i = 0; i < n; ++i) { h->a[i] = h->c[i]; ((bf16_t*)h->b)[i] = (bf16_t)h->c[i]; }      // every byte of every buffer is ours
    h->d[0] = (double)h->a[n - 1];
    CHECK(h->d[0] == (double)(n - 1));
    delete h;
    live(&c1, &b1);
    CHECK(c1 == c0 && b1 == b0);
    printf("arena_check: ok (%d refused allocations, one create + delete)\n", N_ALLOC);
    return 0;
}
