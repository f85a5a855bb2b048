// Host-only known answers for pq::BasicStream (piqp_amd/csrc/common.hpp), the owner of every hipStream_t in the library: the class is instantiated with a create /
// destroy pair that only counts, so no device and no HIP runtime is needed.  Built with -fsanitize=address,undefined by tests/test_stream_raii.py.
#include <cstdint>
#include <cstdio>
#include <set>
#include <stdexcept>
#include <utility>

#include "../../piqp_amd/csrc/common.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

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

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks passed\n");
    return 0;
}
