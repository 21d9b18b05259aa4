// tests/mem_ledger_main.cpp -- MemLedger (ekf_vio_amd/csrc/mem.h) against a malloc backend, as a plain program for a host sanitizer
// (tests/test_mem_cpu.py compiles it with -fsanitize=address,undefined and requires exit status 0).
// The backend keeps the set of live pointers and aborts on a free of a pointer it does not hold, which covers a second free too.
#define EKFVIO_TEST_HOOKS  // fail_nth
#include "../ekf_vio_amd/csrc/mem.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>

namespace {
struct Live {
    MemKind kind;
    size_t bytes;
};
std::map<void*, Live> g_live;
std::vector<void*> g_freed;  // in order
int g_calls = 0;             // allocate calls that reached the backend

int fake_allocate(MemKind kind, size_t bytes, void** out) {
    g_calls++;
    void* p = malloc(bytes ? bytes : 1);
    if (!p) abort();
    g_live[p] = {kind, bytes};
    *out = p;
    return MEM_OK;
}
void fake_free(MemKind kind, void* p, size_t bytes) {
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second.kind != kind || it->second.bytes != bytes) {
        fprintf(stderr, "free of %p: not live, or not as it was allocated\n", p);
        abort();
    }
    g_live.erase(it);
    g_freed.push_back(p);
    free(p);
}
const MemBackend kFake = {fake_allocate, fake_free};

int g_failed = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

int64_t live_of(const MemLedger& m) {
    int64_t n = 0;
    for (int k = 0; k < MEM_KINDS; k++) n += m.counts((MemKind)k).live;
    return n;
}
int64_t acquired_of(const MemLedger& m) {
    int64_t n = 0;
    for (int k = 0; k < MEM_KINDS; k++) n += m.counts((MemKind)k).acquired;
    return n;
}
int64_t released_of(const MemLedger& m) {
    int64_t n = 0;
    for (int k = 0; k < MEM_KINDS; k++) n += m.counts((MemKind)k).released;
    return n;
}

// A script shaped like create_body + klt_alloc + fast_alloc: 70 acquisitions of mixed kinds and types into the fields of a struct, each
// behind an early return.  Returns the index of the acquisition that failed, or -1.
const int SCRIPT = 70;
struct Fields {
    float* f32[40] = {nullptr};
    unsigned char* u8[20] = {nullptr};
    int* host[10] = {nullptr};
};
int script(MemLedger& m, Fields& s) {
    int i = 0;
    for (int k = 0; k < 30; k++, i++)
        if (m.acquire(&s.f32[k], sizeof(float) * (size_t)(k + 1) * 3, MEM_DEVICE) != MEM_OK) return i;
    if (m.acquire(&s.host[0], 64, MEM_PINNED_COHERENT) != MEM_OK) return i;
    i++;
    if (m.acquire(&s.host[1], 4096, MEM_PINNED_COHERENT) != MEM_OK) return i;
    i++;
    if (m.acquire(&s.host[2], 200, MEM_PINNED) != MEM_OK) return i;
    i++;
    for (int k = 0; k < 20; k++, i++)
        if (m.acquire(&s.u8[k], (size_t)1000 + k, MEM_DEVICE) != MEM_OK) return i;
    if (m.acquire(&s.host[3], 19216, MEM_PINNED_MAPPED) != MEM_OK) return i;
    i++;
    for (int k = 30; k < 40; k++, i++)
        if (m.acquire(&s.f32[k], sizeof(float) * (size_t)k, MEM_DEVICE) != MEM_OK) return i;
    for (int k = 4; k < 10; k++, i++)
        if (m.acquire(&s.host[k], 16, MEM_PINNED_MAPPED) != MEM_OK) return i;
    return i == SCRIPT ? -1 : -2;
}
void* field(Fields& s, int i) {  // the slot acquisition i of the script fills
    if (i < 30) return s.f32[i];
    if (i < 33) return s.host[i - 30];
    if (i < 53) return s.u8[i - 33];
    if (i == 53) return s.host[3];
    if (i < 64) return s.f32[30 + i - 54];
    return s.host[4 + i - 64];
}

void test_failure_at_every_step() {
    {
        MemLedger m(kFake);
        Fields s;
        CHECK(script(m, s) == -1);
        CHECK(live_of(m) == SCRIPT && (int64_t)g_live.size() == SCRIPT);
        CHECK(m.counts(MEM_DEVICE).live == 60 && m.counts(MEM_PINNED).live == 1 && m.counts(MEM_PINNED_MAPPED).live == 7 &&
              m.counts(MEM_PINNED_COHERENT).live == 2);
        CHECK(m.counts(MEM_PINNED).live_bytes == 200 && m.counts(MEM_PINNED_COHERENT).live_bytes == 64 + 4096);
    }
    CHECK(g_live.empty());
    for (int k = 1; k <= SCRIPT; k++) {
        MemLedger m(kFake);
        Fields s;
        const int calls = g_calls;
        m.fail_nth(k);
        const int at = script(m, s);
        CHECK(at == k - 1);
        CHECK(field(s, k - 1) == nullptr);       // the failing acquire leaves its slot null
        CHECK(g_calls - calls == k - 1);          // ... without calling the backend
        CHECK(live_of(m) == k - 1 && acquired_of(m) == k - 1);
        m.release_all();
        for (int kind = 0; kind < MEM_KINDS; kind++) CHECK(m.counts((MemKind)kind).live == 0 && m.counts((MemKind)kind).live_bytes == 0);
        CHECK(released_of(m) == k - 1);           // releases ever == acquisitions that succeeded
        CHECK(g_live.empty());
        // the injection fires once: the same ledger now takes the whole script
        Fields again;
        CHECK(script(m, again) == -1 && live_of(m) == SCRIPT);
    }
    CHECK(g_live.empty());
}

void test_grow() {
    MemLedger m(kFake);
    float *a = nullptr, *b = nullptr;
    CHECK(m.acquire(&a, 100, MEM_DEVICE) == MEM_OK && m.acquire(&b, 50, MEM_DEVICE) == MEM_OK);
    const MemCounts before = m.counts(MEM_DEVICE);
    void* old = a;
    g_freed.clear();
    CHECK(m.acquire(&a, 400, MEM_DEVICE) == MEM_OK);
    CHECK(a && g_live.count(a) && g_live[a].bytes == 400);
    CHECK(m.counts(MEM_DEVICE).live == before.live && m.counts(MEM_DEVICE).released == before.released + 1 &&
          m.counts(MEM_DEVICE).acquired == before.acquired + 1 && m.counts(MEM_DEVICE).live_bytes == before.live_bytes + 300);
    CHECK(g_freed.size() == 1 && g_freed[0] == old);
    // a failed grow: the slot is null, one allocation fewer, the old pointer freed exactly once (a second free would abort in the backend)
    old = a;
    g_freed.clear();
    m.fail_nth(1);
    CHECK(m.acquire(&a, 800, MEM_DEVICE) == MEM_ERR_OUT_OF_MEMORY);
    CHECK(a == nullptr && m.counts(MEM_DEVICE).live == before.live - 1);
    CHECK(g_freed.size() == 1 && g_freed[0] == old && !g_live.count(old));
    m.release_all();
    CHECK(g_freed.size() == 2 && g_live.empty());
}

void test_swap() {
    MemLedger m(kFake);
    float *p = nullptr, *p2 = nullptr, *q = nullptr;
    CHECK(m.acquire(&p, 64, MEM_DEVICE) == MEM_OK && m.acquire(&p2, 64, MEM_DEVICE) == MEM_OK && m.acquire(&q, 8, MEM_DEVICE) == MEM_OK);
    void *was_p = p, *was_p2 = p2;
    std::swap(p, p2);  // as launch_predict exchanges P / P2
    g_freed.clear();
    CHECK(m.release(&p) == MEM_OK && p == nullptr);
    CHECK(g_freed.size() == 1 && g_freed[0] == was_p2);
    m.release_all();
    CHECK(g_freed.size() == 3 && std::count(g_freed.begin(), g_freed.end(), was_p) == 1 && std::count(g_freed.begin(), g_freed.end(), was_p2) == 1);
    CHECK(g_live.empty());
}

void test_foreign_pointer() {
    MemLedger m(kFake), other(kFake);
    float *mine = nullptr, *theirs = nullptr;
    CHECK(m.acquire(&mine, 16, MEM_DEVICE) == MEM_OK && other.acquire(&theirs, 16, MEM_DEVICE) == MEM_OK);
    int on_stack = 0;
    int* stray = &on_stack;
    g_freed.clear();
    const int calls = g_calls;
    CHECK(m.acquire(&theirs, 32, MEM_DEVICE) == MEM_ERR_FOREIGN);
    CHECK(m.acquire(&stray, 32, MEM_DEVICE) == MEM_ERR_FOREIGN);
    CHECK(m.release(&stray) == MEM_ERR_FOREIGN);
    CHECK(g_freed.empty() && g_calls == calls);  // reported: nothing freed, nothing allocated
    CHECK(stray == &on_stack && theirs && g_live.count(theirs) && live_of(m) == 1 && live_of(other) == 1);
}

bool early_return(bool leave) {  // the shape of a test hook: temporaries on a stack ledger, a return in the middle
    MemLedger tmp(kFake);
    float *a = nullptr, *b = nullptr, *c = nullptr;
    if (tmp.acquire(&a, 10, MEM_DEVICE) != MEM_OK || tmp.acquire(&b, 20, MEM_DEVICE) != MEM_OK || tmp.acquire(&c, 30, MEM_PINNED) != MEM_OK) return false;
    if (g_live.size() != 3) return false;
    if (leave) return true;
    a[0] = 1.f;
    return true;
}
void test_scope_exit() {
    CHECK(g_live.empty());
    CHECK(early_return(true));
    CHECK(g_live.empty());
}

void test_reverse_order() {
    std::vector<void*> order;
    {
        MemLedger m(kFake);
        int* s[6] = {nullptr};
        for (int i = 0; i < 6; i++) {
            CHECK(m.acquire(&s[i], 8 + i, i % 2 ? MEM_PINNED : MEM_DEVICE) == MEM_OK);
            order.push_back(s[i]);
        }
        CHECK(m.release(&s[2]) == MEM_OK);  // taken out of the middle: the rest keep their order
        order.erase(order.begin() + 2);
        g_freed.clear();
    }  // (the destructor is release_all)
    std::reverse(order.begin(), order.end());
    CHECK(g_freed == order);
}
}  // namespace

int main() {
    test_failure_at_every_step();
    test_grow();
    test_swap();
    test_foreign_pointer();
    test_scope_exit();
    test_reverse_order();
    CHECK(g_live.empty());
    if (g_failed) {
        fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    printf("mem ledger: ok\n");
    return 0;
}
