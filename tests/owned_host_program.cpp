// Stand-alone check of csrc/gas_owned.h against a fake runtime (malloc / free): built by tests/test_owned_host_program.py
// with the sanitizers and run as a child process.  Usage: owned_host_program <case>; prints "ok" and exits 0, or prints
// what did not hold and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <thread>

#include "gas_owned.h"

namespace {

// Every object is a malloc block, remembered per kind: a free of something not live in its kind (twice, or through the
// wrong call) is counted, not carried out.  The k-th allocation of any kind can be made to fail.
struct Fake {
	using status = int;
	struct ev_t {
		int unused;
	};
	using event = ev_t *;
	static constexpr status misuse = -2;
	static std::mutex mu;
	static std::set<void *> live[3];
	static long allocs, frees, bad_frees, fail_at;

	static status make(int kind, void **p, size_t bytes) {
		std::lock_guard<std::mutex> lk(mu);
		if (++allocs == fail_at) {
			return -1;
		}
		*p = malloc(bytes ? bytes : 1);
		live[kind].insert(*p);
		return 0;
	}
	static status unmake(int kind, void *p) {
		std::lock_guard<std::mutex> lk(mu);
		if (live[kind].erase(p) == 0) {
			bad_frees++;
			return -1;
		}
		free(p);
		frees++;
		return 0;
	}
	static size_t count(int kind) {
		std::lock_guard<std::mutex> lk(mu);
		return live[kind].size();
	}
	static size_t total() {
		return count(0) + count(1) + count(2);
	}
	static void reset() {
		allocs = frees = bad_frees = fail_at = 0;
	}

	static status device_alloc(void **p, size_t bytes) {
		return make(0, p, bytes);
	}
	static status device_free(void *p) {
		return unmake(0, p);
	}
	static status pinned_alloc(void **p, size_t bytes) {
		return make(1, p, bytes);
	}
	static status pinned_free(void *p) {
		return unmake(1, p);
	}
	static status event_create(event *e, unsigned) {
		return make(2, reinterpret_cast<void **>(e), sizeof(ev_t));
	}
	static status event_destroy(event e) {
		return unmake(2, e);
	}
};
std::mutex Fake::mu;
std::set<void *> Fake::live[3];
long Fake::allocs, Fake::frees, Fake::bad_frees, Fake::fail_at;

using Owner = gas_owned<Fake>;

int failures = 0;
#define CHECK(cond)                                             \
	do {                                                        \
		if (!(cond)) {                                          \
			printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
			failures++;                                         \
		}                                                       \
	} while (0)

void case_basic() {
	Fake::reset();
	{
		Owner o;
		float *a = nullptr;
		void *b = nullptr;
		uint8_t *c = nullptr;
		double *h0 = nullptr;
		uint32_t *h1 = nullptr;
		Fake::event e0 = nullptr, e1 = nullptr;
		CHECK(o.alloc(a, 100) == 0 && o.alloc(b, 33) == 0 && o.alloc(c, 7) == 0);
		CHECK(o.alloc(h0, 5, Owner::PINNED) == 0 && o.alloc(h1, 9, Owner::PINNED) == 0);
		CHECK(o.make_event(e0, 0) == 0 && o.make_event(e1, 2) == 0);
		memset(a, 1, 100 * sizeof(float)); // the sizes are in elements, bytes for void *: the sanitizer sees a short block
		memset(b, 1, 33);
		memset(h0, 1, 5 * sizeof(double));
		CHECK(o.live() == 7 && Fake::count(0) == 3 && Fake::count(1) == 2 && Fake::count(2) == 2);
		CHECK(o.drop(b) && o.drop(h0) && o.drop(e1));
		CHECK(!b && !h0 && !e1 && o.live() == 4 && Fake::frees == 3);
		o.release_all();
		CHECK(o.live() == 0 && Fake::total() == 0 && Fake::frees == 7);
		o.release_all();
		CHECK(Fake::frees == 7);
	}
	CHECK(Fake::frees == 7 && Fake::allocs == 7 && Fake::bad_frees == 0);
}

void case_grow() {
	Fake::reset();
	Owner o;
	for (const Owner::Kind kind : { Owner::DEVICE, Owner::PINNED }) {
		const int k = kind == Owner::DEVICE ? 0 : 1;
		float *p = nullptr;
		uint32_t cap = 0;
		CHECK(o.grow(p, cap, 8, 1, kind) == 0 && p && cap == 8 && Fake::count(k) == 1);
		// hit: nothing changes
		float *const was = p;
		const long allocs = Fake::allocs, frees = Fake::frees;
		CHECK(o.grow(p, cap, 8, 1, kind) == 0 && o.grow(p, cap, 3, 1, kind) == 0);
		CHECK(p == was && cap == 8 && Fake::allocs == allocs && Fake::frees == frees);
		// miss: the old object is freed, the new one recorded with the new capacity (`per` elements per unit)
		CHECK(o.grow(p, cap, 16, 3, kind) == 0 && p && cap == 16);
		memset(p, 1, 16 * 3 * sizeof(float));
		CHECK(Fake::frees == frees + 1 && Fake::allocs == allocs + 1 && o.live() == 1 && Fake::count(k) == 1);
		// the allocation fails: null, capacity 0, the old object freed once
		Fake::fail_at = Fake::allocs + 1;
		CHECK(o.grow(p, cap, 32, 1, kind) != 0 && !p && cap == 0);
		CHECK(Fake::frees == frees + 2 && o.live() == 0 && Fake::total() == 0);
		// and the next call starts over
		CHECK(o.grow(p, cap, 4, 1, kind) == 0 && p && cap == 4 && o.drop(p));
	}
	size_t bytes = 0;
	void *v = nullptr;
	CHECK(o.grow(v, bytes, 48) == 0 && bytes == 48);
	memset(v, 1, 48);
	o.release_all();
	CHECK(Fake::total() == 0 && Fake::bad_frees == 0 && Fake::frees == Fake::allocs - 2);
}

// The shape of gas_ctx_create: a run of allocations that stops at the first failure.
int create_like(Owner &o, float *&a, uint32_t *&b, void *&c, float *&h, Fake::event &e0, Fake::event &e1, uint8_t *&d, float *&g, size_t &g_cap) {
	int s = o.alloc(a, 64);
	s = s ? s : o.alloc(b, 16);
	s = s ? s : o.alloc(c, 100);
	s = s ? s : o.alloc(h, 8, Owner::PINNED);
	s = s ? s : o.make_event(e0, 0);
	s = s ? s : o.make_event(e1, 0);
	s = s ? s : o.alloc(d, 1);
	s = s ? s : o.grow(g, g_cap, 10);
	s = s ? s : o.grow(g, g_cap, 20);
	return s;
}

void case_fail_each() {
	const long n = 9;
	for (int by_destructor = 0; by_destructor < 2; by_destructor++) {
		for (long k = 1; k <= n + 1; k++) { // n + 1: none fails
			Fake::reset();
			Fake::fail_at = k;
			{
				Owner o;
				float *a = nullptr, *h = nullptr, *g = nullptr;
				uint32_t *b = nullptr;
				void *c = nullptr;
				uint8_t *d = nullptr;
				Fake::event e0 = nullptr, e1 = nullptr;
				size_t g_cap = 0;
				const int s = create_like(o, a, b, c, h, e0, e1, d, g, g_cap);
				CHECK((s != 0) == (k <= n));
				CHECK(Fake::allocs == (k <= n ? k : n));
				CHECK(o.live() == Fake::total());
				if (!by_destructor) {
					o.release_all();
					CHECK(o.live() == 0 && Fake::total() == 0);
				}
			}
			CHECK(Fake::total() == 0 && Fake::bad_frees == 0);
			CHECK(Fake::frees == Fake::allocs - (k <= n ? 1 : 0)); // every object that came to exist, once
		}
	}
}

void case_refuse() {
	Fake::reset();
	Owner o, other;
	float *null_p = nullptr;
	Fake::event null_e = nullptr;
	CHECK(o.drop(null_p) && o.drop(null_e) && Fake::frees == 0);
	// a pointer the owner does not hold: not freed, not nulled
	float *foreign = static_cast<float *>(malloc(16));
	float *const foreign_was = foreign;
	CHECK(!o.drop(foreign) && foreign == foreign_was && Fake::frees == 0 && Fake::bad_frees == 0);
	free(foreign);
	float *theirs = nullptr;
	CHECK(other.alloc(theirs, 4) == 0);
	float *const theirs_was = theirs;
	CHECK(!o.drop(theirs) && theirs == theirs_was && other.live() == 1 && Fake::frees == 0);
	// dropped twice through a second name: the second is refused
	float *alias = theirs;
	CHECK(other.drop(theirs) && !other.drop(alias) && Fake::frees == 1 && Fake::bad_frees == 0);
	// allocating over a live pointer is refused before anything is allocated
	float *mine = nullptr;
	CHECK(o.alloc(mine, 4) == 0);
	float *const mine_was = mine;
	const long allocs = Fake::allocs;
	CHECK(o.alloc(mine, 8) == Fake::misuse && o.alloc(mine, 8, Owner::PINNED) == Fake::misuse);
	CHECK(mine == mine_was && Fake::allocs == allocs && o.live() == 1);
}

int scope_body(bool leave_early) {
	Owner tmp;
	float *a = nullptr, *b = nullptr, *h = nullptr;
	Fake::event e0 = nullptr, e1 = nullptr;
	if (tmp.alloc(a, 10) || tmp.alloc(b, 20) || tmp.make_event(e0, 0)) {
		return -1;
	}
	if (leave_early) {
		return 1;
	}
	if (tmp.alloc(h, 5, Owner::PINNED) || tmp.make_event(e1, 0)) {
		return -1;
	}
	return 0;
}

void case_scope() {
	Fake::reset();
	CHECK(scope_body(true) == 1 && Fake::total() == 0 && Fake::frees == 3);
	CHECK(scope_body(false) == 0 && Fake::total() == 0 && Fake::frees == 8);
	Fake::fail_at = Fake::allocs + 2;
	CHECK(scope_body(false) == -1 && Fake::total() == 0 && Fake::bad_frees == 0);
}

void case_threads() {
	Fake::reset();
	Owner o;
	auto work = [&o](int seed) {
		float *g = nullptr;
		size_t g_cap = 0;
		for (int i = 0; i < 2000; i++) {
			float *d = nullptr;
			uint32_t *h = nullptr;
			Fake::event e = nullptr;
			bool ok = o.alloc(d, 8 + (i + seed) % 5) == 0 && o.alloc(h, 4, Owner::PINNED) == 0 && o.make_event(e, 0) == 0;
			ok = ok && o.grow(g, g_cap, (size_t)(i % 64) + 1) == 0;
			ok = ok && o.drop(d) && o.drop(e);
			if (i % 3 != 0) {
				ok = ok && o.drop(h); // every third stays for release_all
			}
			if (!ok) {
				std::lock_guard<std::mutex> lk(Fake::mu);
				failures++;
			}
		}
	};
	std::thread t0(work, 0), t1(work, 1);
	t0.join();
	t1.join();
	CHECK(o.live() == Fake::total() && o.live() == 2 * (667 + 1)); // the pinned blocks kept, and each thread's grown buffer
	o.release_all();
	CHECK(o.live() == 0 && Fake::total() == 0 && Fake::bad_frees == 0 && Fake::frees == Fake::allocs);
}

} // namespace

int main(int argc, char **argv) {
	const std::string which = argc > 1 ? argv[1] : "";
	if (which == "basic") {
		case_basic();
	} else if (which == "grow") {
		case_grow();
	} else if (which == "fail_each") {
		case_fail_each();
	} else if (which == "refuse") {
		case_refuse();
	} else if (which == "scope") {
		case_scope();
	} else if (which == "threads") {
		case_threads();
	} else {
		printf("unknown case\n");
		return 2;
	}
	if (failures == 0) {
		printf("ok\n");
	}
	return failures ? 1 : 0;
}
