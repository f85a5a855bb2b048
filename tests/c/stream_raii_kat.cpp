// Host-only known answers for pq::BasicStream and pq::BasicEvent (piqp_amd/csrc/common.hpp), the owners of every hipStream_t and hipEvent_t in the library: the classes
// are instantiated with create / destroy pairs that only count, so no device and no HIP runtime is needed.  Built with -fsanitize=address,undefined by
// tests/test_stream_raii.py.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../piqp_amd/csrc/common.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

std::vector<std::string> seq;  // what was released, in order: the stream's, the event's and the stand-ins' destroys all log here

struct CountingApi {
    static int created, destroyed, bad_destroys, last_device;
    static bool fail_create;
    static std::set<hipStream_t> live;
    static hipStream_t create(int device)
    {
        if (fail_create) throw std::runtime_error("create failed");
        last_device = device;
        hipStream_t s = reinterpret_cast<hipStream_t>(static_cast<std::uintptr_t>(0x1000 + 16 * ++created));
        live.insert(s);
        return s;
    }
    static void destroy(int device, hipStream_t s) noexcept
    {
        ++destroyed;
        seq.push_back("stream");
        last_device = device;
        if (s == nullptr || live.erase(s) != 1) ++bad_destroys;  // a null handle, one destroyed before, or one this Api never made or was told about
    }
    static void reset() { created = destroyed = bad_destroys = 0; last_device = -1; fail_create = false; live.clear(); }
};
int CountingApi::created = 0, CountingApi::destroyed = 0, CountingApi::bad_destroys = 0, CountingApi::last_device = -1;
bool CountingApi::fail_create = false;
std::set<hipStream_t> CountingApi::live;

using Api = CountingApi;
using S = pq::BasicStream<CountingApi>;

struct CountingEventApi {
    static int created, destroyed, bad_destroys;
    static unsigned last_flags;
    static int fail_at;  // the create with this number (1-based, since reset) throws; 0: none
    static std::set<hipEvent_t> live;
    static hipEvent_t create(unsigned flags)
    {
        if (fail_at && created + 1 == fail_at) throw std::runtime_error("event create failed");
        last_flags = flags;
        hipEvent_t e = reinterpret_cast<hipEvent_t>(static_cast<std::uintptr_t>(0x8000 + 16 * ++created));
        live.insert(e);
        return e;
    }
    static void destroy(hipEvent_t e) noexcept
    {
        ++destroyed;
        seq.push_back("event");
        if (e == nullptr || live.erase(e) != 1) ++bad_destroys;  // a null handle, one destroyed before, or one this Api never made
    }
    static void reset() { created = destroyed = bad_destroys = 0; last_flags = ~0u; fail_at = 0; live.clear(); seq.clear(); }
};
int CountingEventApi::created = 0, CountingEventApi::destroyed = 0, CountingEventApi::bad_destroys = 0, CountingEventApi::fail_at = 0;
unsigned CountingEventApi::last_flags = ~0u;
std::set<hipEvent_t> CountingEventApi::live;

using EApi = CountingEventApi;
using E = pq::BasicEvent<CountingEventApi>;

struct ThrowsAfterTwoEvents {
    E a, b;
    ThrowsAfterTwoEvents() : a(0), b(2) { throw std::runtime_error("the rest of the constructor failed"); }
};
struct TwoEvents {
    E a, b;
    TwoEvents() : a(0), b(0) {}
};

// the one declaration order of every handle type: buffers, events, a communicator, the streams last
struct BufferStandIn {
    ~BufferStandIn() { seq.push_back("buffer"); }
};
struct CommStandIn {};
struct CommDeleter {
    void operator()(CommStandIn* c) const noexcept { seq.push_back("communicator"); delete c; }
};
struct HandleShape {
    BufferStandIn buf;
    E ev{0};
    std::unique_ptr<CommStandIn, CommDeleter> comm{new CommStandIn};
    S st{1};
};

struct ThrowsAfterTheStream {
    S st;
    ThrowsAfterTheStream() : st(3) { throw std::runtime_error("the rest of the constructor failed"); }
};

// the shape of the multifrontal engine's constructor: an adopted stream goes back to the caller, un-destroyed, when the rest of the constructor fails
struct AdoptsOrGivesBack {
    S st;
    AdoptsOrGivesBack(hipStream_t adopt, bool fail)
    {
        st = S(5, adopt);
        try {
            if (fail) throw std::runtime_error("the rest of the constructor failed");
        } catch (...) {
            (void)st.release();
            throw;
        }
    }
};

}  // namespace

int main()
{
    Api::reset();
    {   // empty: nothing to create, nothing to destroy
        S e;
        CHECK(e.get() == nullptr && !e);
        CHECK(e.release() == nullptr);
    }
    CHECK(Api::created == 0 && Api::destroyed == 0);

    {   // construct / destroy: one of each, on the stream's device
        S a(2);
        CHECK(Api::created == 1 && Api::last_device == 2 && a.get() != nullptr && static_cast<hipStream_t>(a) == a.get());
        CHECK(Api::destroyed == 0);
        Api::last_device = -1;
    }
    CHECK(Api::created == 1 && Api::destroyed == 1 && Api::last_device == 2 && Api::live.empty());

    Api::reset();
    {   // move construction: the handle changes owner, the source is empty, one destroy in all
        S a(0);
        const hipStream_t h = a.get();
        S b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == h && Api::destroyed == 0);
    }
    CHECK(Api::created == 1 && Api::destroyed == 1 && Api::bad_destroys == 0);

    Api::reset();
    {   // move assignment: what the target held is destroyed at once, what it takes later; onto itself: nothing
        S a(0), b(1);
        const hipStream_t hb = b.get();
        a = std::move(b);
        CHECK(Api::destroyed == 1 && Api::last_device == 0 && a.get() == hb && b.get() == nullptr);
        S& self = a;
        a = std::move(self);
        CHECK(Api::destroyed == 1 && a.get() == hb);
        S e;
        e = std::move(a);  // into an empty one: no destroy
        CHECK(Api::destroyed == 1 && e.get() == hb && a.get() == nullptr);
        Api::last_device = -1;
    }
    CHECK(Api::created == 2 && Api::destroyed == 2 && Api::last_device == 1 && Api::bad_destroys == 0 && Api::live.empty());

    Api::reset();
    hipStream_t kept = nullptr;
    {   // release: the caller owns it, the destructor does nothing
        S a(4);
        kept = a.release();
        CHECK(kept != nullptr && a.get() == nullptr);
    }
    CHECK(Api::created == 1 && Api::destroyed == 0 && Api::live.count(kept) == 1);
    {   // adopt: takes ownership of an existing stream with its device
        S b(7, kept);
        CHECK(b.get() == kept && Api::created == 1);
    }
    CHECK(Api::destroyed == 1 && Api::last_device == 7 && Api::bad_destroys == 0 && Api::live.empty());

    Api::reset();
    try {   // a constructor that throws after its stream exists: exactly one destroy
        ThrowsAfterTheStream t;
        CHECK(false);
    } catch (const std::runtime_error&) {
    }
    CHECK(Api::created == 1 && Api::destroyed == 1 && Api::last_device == 3 && Api::bad_destroys == 0 && Api::live.empty());

    Api::reset();
    Api::fail_create = true;
    try {   // the create itself fails: nothing to destroy
        S a(0);
        CHECK(false);
    } catch (const std::runtime_error&) {
    }
    CHECK(Api::created == 0 && Api::destroyed == 0);

    Api::reset();
    {   // adopt, fail, give back: the caller's holder still owns the one stream; adopt and succeed: the new owner destroys it, the caller lets go
        S caller(5);
        const hipStream_t h = caller.get();
        try {
            AdoptsOrGivesBack x(caller.get(), true);
            CHECK(false);
        } catch (const std::runtime_error&) {
        }
        CHECK(Api::destroyed == 0 && caller.get() == h);
        {
            AdoptsOrGivesBack y(caller.get(), false);
            (void)caller.release();
            CHECK(y.st.get() == h && Api::destroyed == 0);
        }
        CHECK(Api::destroyed == 1);
    }
    CHECK(Api::created == 1 && Api::destroyed == 1 && Api::bad_destroys == 0 && Api::live.empty());

    // ---- pq::BasicEvent
    EApi::reset();
    {   // empty: no calls
        E e;
        CHECK(e.get() == nullptr && !e);
    }
    CHECK(EApi::created == 0 && EApi::destroyed == 0 && seq.empty());

    {   // construct / destroy: one of each, with the flags asked for
        E a(2);
        CHECK(EApi::created == 1 && EApi::last_flags == 2u && a.get() != nullptr && static_cast<hipEvent_t>(a) == a.get());
        CHECK(EApi::destroyed == 0);
    }
    CHECK(EApi::created == 1 && EApi::destroyed == 1 && EApi::bad_destroys == 0 && EApi::live.empty());

    EApi::reset();
    {   // move construction and move assignment into an empty one: nothing created, nothing destroyed, the source is empty
        E a(0);
        const hipEvent_t h = a.get();
        E b(std::move(a));
        CHECK(a.get() == nullptr && b.get() == h && EApi::created == 1 && EApi::destroyed == 0);
        E c;
        c = std::move(b);
        CHECK(b.get() == nullptr && c.get() == h && EApi::created == 1 && EApi::destroyed == 0);
    }
    CHECK(EApi::created == 1 && EApi::destroyed == 1 && EApi::bad_destroys == 0 && EApi::live.empty());

    EApi::reset();
    {   // move assignment onto a live event: the old one is destroyed exactly once, at once; onto itself: nothing
        E a(0), b(0);
        const hipEvent_t ha = a.get(), hb = b.get();
        a = std::move(b);
        CHECK(EApi::destroyed == 1 && EApi::live.count(ha) == 0 && EApi::live.count(hb) == 1 && a.get() == hb && b.get() == nullptr);
        E& self = a;
        a = std::move(self);
        CHECK(EApi::destroyed == 1 && a.get() == hb);
    }
    CHECK(EApi::created == 2 && EApi::destroyed == 2 && EApi::bad_destroys == 0 && EApi::live.empty());

    EApi::reset();
    try {   // a constructor that throws after both events exist: each destroyed once
        ThrowsAfterTwoEvents t;
        CHECK(false);
    } catch (const std::runtime_error&) {
    }
    CHECK(EApi::created == 2 && EApi::destroyed == 2 && EApi::bad_destroys == 0 && EApi::live.empty());

    EApi::reset();
    EApi::fail_at = 2;
    try {   // the second event's create throws: the first is destroyed, nothing else
        TwoEvents t;
        CHECK(false);
    } catch (const std::runtime_error&) {
    }
    CHECK(EApi::created == 1 && EApi::destroyed == 1 && EApi::bad_destroys == 0 && EApi::live.empty());

    Api::reset();
    EApi::reset();
    {
        HandleShape h;
        CHECK(seq.empty());
    }
    CHECK((seq == std::vector<std::string>{"stream", "communicator", "event", "buffer"}));
    CHECK(Api::bad_destroys == 0 && EApi::bad_destroys == 0 && Api::live.empty() && EApi::live.empty());

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
