// ekf_vio_amd/csrc/mem.h — everything that OWNS: the device and pinned memory of a handle, or of one test hook's call.
// Standard headers only (no HIP, no project header), like plan.h: the ledger is checked under a host sanitizer against a malloc backend
// (tests/mem_ledger_main.cpp, tests/test_mem_cpu.py).  The library's backend (api.hip, hip_mem_backend) is the only code under csrc/ that
// calls the runtime's allocation functions.
// A MemLedger records what was acquired through it BY POINTER VALUE, not by the field that holds the pointer: P / P2, mu / mu_next and what
// remove_applied exchanges swap between fields during a run, and whichever field holds a pointer at the end, it is released once.
#ifndef EKFVIO_MEM_H_
#define EKFVIO_MEM_H_
#include <stddef.h>
#include <stdint.h>

#include <vector>

enum MemKind {
    MEM_DEVICE = 0,
    MEM_PINNED,           // page-locked host memory (default flags)
    MEM_PINNED_MAPPED,    // ... mapped into the device's address space
    MEM_PINNED_COHERENT,  // ... mapped and coherent: words a kernel publishes while the host polls
    MEM_KINDS
};
enum MemError {
    MEM_OK = 0,
    MEM_ERR_OUT_OF_MEMORY = 2,  // what fail_nth reports (the runtime's own out-of-memory code: api.hip asserts the two agree)
    MEM_ERR_FOREIGN = -1,       // acquire / release on a non-null slot this ledger does not own: a programming error, nothing is freed
};

// allocate: 0 and *out on success, otherwise its own error code (which acquire hands back) and *out untouched
struct MemBackend {
    int (*allocate)(MemKind kind, size_t bytes, void** out);
    void (*free)(MemKind kind, void* p, size_t bytes);
};

struct MemCounts {
    int64_t live = 0, live_bytes = 0;     // held now
    int64_t acquired = 0, released = 0;   // ever (successful acquisitions only: live == acquired - released)
};

class MemLedger {
public:
    explicit MemLedger(const MemBackend& backend) : backend_(backend) {}
    ~MemLedger() { release_all(); }  // a ledger on the stack is scratch memory released on every return path
    MemLedger(const MemLedger&) = delete;
    MemLedger& operator=(const MemLedger&) = delete;

    // *slot becomes `bytes` of `kind`.  A non-null *slot must be this ledger's and is released first (the "grow" of a buffer).  On failure
    // *slot is null, nothing else has changed and the backend's error comes back.
    template <class T>
    int acquire(T** slot, size_t bytes, MemKind kind) {
        if (*slot && find(*slot) < 0) return MEM_ERR_FOREIGN;
        release(slot);
#ifdef EKFVIO_TEST_HOOKS
        if (fail_in_ > 0 && --fail_in_ == 0) return MEM_ERR_OUT_OF_MEMORY;
#endif
        void* p = nullptr;
        const int rc = backend_.allocate(kind, bytes, &p);
        if (rc != MEM_OK) return rc;
        live_.push_back({p, bytes, kind});
        counts_[kind].live++, counts_[kind].live_bytes += (int64_t)bytes, counts_[kind].acquired++;
        *slot = static_cast<T*>(p);
        return MEM_OK;
    }
    // frees and nulls the slot (a null slot: nothing to do)
    template <class T>
    int release(T** slot) {
        if (!*slot) return MEM_OK;
        const int i = find(*slot);
        if (i < 0) return MEM_ERR_FOREIGN;
        free_entry(live_[i]);
        live_.erase(live_.begin() + i);
        *slot = nullptr;
        return MEM_OK;
    }
    // everything still held, in reverse order of acquisition (the fields that pointed at it are the caller's to forget)
    void release_all() {
        while (!live_.empty()) {
            free_entry(live_.back());
            live_.pop_back();
        }
    }
    const MemCounts& counts(MemKind kind) const { return counts_[kind]; }
#ifdef EKFVIO_TEST_HOOKS
    // the k-th acquisition from now reports MEM_ERR_OUT_OF_MEMORY without calling the backend, once; 0 disarms
    void fail_nth(int k) { fail_in_ = k > 0 ? k : 0; }
#endif

private:
    struct Entry {
        void* p;
        size_t bytes;
        MemKind kind;
    };
    int find(const void* p) const {  // a handle holds under a hundred entries, and nothing per frame comes through here
        for (size_t i = live_.size(); i-- > 0;)
            if (live_[i].p == p) return (int)i;
        return -1;
    }
    void free_entry(const Entry& e) {
        backend_.free(e.kind, e.p, e.bytes);
        counts_[e.kind].live--, counts_[e.kind].live_bytes -= (int64_t)e.bytes, counts_[e.kind].released++;
    }
    MemBackend backend_;
    std::vector<Entry> live_;  // in order of acquisition
    MemCounts counts_[MEM_KINDS];
#ifdef EKFVIO_TEST_HOOKS
    int fail_in_ = 0;
#endif
};
#endif  // EKFVIO_MEM_H_
