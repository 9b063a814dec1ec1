// gas_owned.h -- one owner for device buffers, pinned host buffers and events.
//
// Whatever is allocated through a gas_owned is recorded in it and freed by drop(), by release_all() or by the
// destructor, whichever comes first: nothing it handed out leaks and nothing is freed twice.  The caller keeps the raw
// pointers (they are passed to kernels by value); the owner only remembers them.  A local instance is the scope guard
// of a function's temporaries.
//
// The runtime is reached through the policy type P alone, so this header includes no HIP and a test can supply a fake:
//   using status = ...;  using event = ...;           // status{} is success; an event handle is a pointer
//   static constexpr status misuse = ...;             // what allocating into a non-null pointer returns
//   static status device_alloc(void **p, size_t bytes);    static status device_free(void *p);
//   static status pinned_alloc(void **p, size_t bytes);    static status pinned_free(void *p);
//   static status event_create(event *e, unsigned flags);  static status event_destroy(event e);
//
// Every member may be called from any thread.  The mutex guards the record only: the runtime calls run outside it.
#pragma once

#include <cstddef>
#include <mutex>
#include <type_traits>
#include <unordered_map>

template <class P>
class gas_owned {
public:
	using status = typename P::status;
	using event = typename P::event;
	enum Kind : unsigned char { DEVICE, PINNED, EVENT };

	~gas_owned() {
		release_all();
	}

	// `count` elements (bytes for void *) of device or pinned host memory.  p must be null: an owned pointer that is
	// overwritten could no longer be dropped.
	template <class T>
	status alloc(T *&p, size_t count, Kind kind = DEVICE) {
		if (p) {
			return P::misuse;
		}
		void *raw = nullptr;
		const size_t bytes = count * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
		const status s = kind == DEVICE ? P::device_alloc(&raw, bytes) : P::pinned_alloc(&raw, bytes);
		if (s == status{}) {
			record(raw, kind);
			p = static_cast<T *>(raw);
		}
		return s;
	}

	status make_event(event &e, unsigned flags) {
		const status s = P::event_create(&e, flags);
		if (s == status{}) {
			record(e, EVENT);
		}
		return s;
	}

	// Frees p, forgets it and nulls the caller's variable; null is a no-op.  A pointer this owner does not hold is
	// refused: nothing is freed, the variable keeps its value and the result is false.  (The status of the free itself
	// is not reported: the runtime refuses only pointers it does not know, and the record rules those out.)
	template <class T>
	bool drop(T *&p) {
		if (!p) {
			return true;
		}
		Kind kind;
		{
			std::lock_guard<std::mutex> lk(mu_);
			const auto it = live_.find(p); // a hash lookup, not a walk: a context holds thousands of streams
			if (it == live_.end()) {
				return false;
			}
			kind = it->second;
			live_.erase(it);
		}
		free_one(p, kind);
		p = nullptr;
		return true;
	}

	// Room for `need` units of `per` elements each behind p, whose capacity in units is cap.  need <= cap changes
	// nothing; otherwise the old buffer is dropped (its contents are not kept), a new one is allocated and cap = need.
	// On failure p is null and cap is 0.  The caller waits for whatever still uses the old buffer first.
	template <class T, class C>
	status grow(T *&p, C &cap, size_t need, size_t per = 1, Kind kind = DEVICE) {
		if (need <= cap) {
			return status{};
		}
		drop(p);
		cap = 0;
		const status s = alloc(p, need * per, kind);
		if (s == status{}) {
			cap = (C)need;
		}
		return s;
	}

	// Frees everything still recorded.  The caller's pointers are left dangling: for the end of their life.
	void release_all() {
		std::unordered_map<const void *, Kind> all;
		{
			std::lock_guard<std::mutex> lk(mu_);
			all.swap(live_);
		}
		for (const auto &kv : all) {
			free_one(kv.first, kv.second);
		}
	}

	size_t live() const {
		std::lock_guard<std::mutex> lk(mu_);
		return live_.size();
	}

private:
	void record(const void *p, Kind kind) {
		std::lock_guard<std::mutex> lk(mu_);
		live_.emplace(p, kind);
	}

	static void free_one(const void *p, Kind kind) {
		void *q = const_cast<void *>(p);
		if (kind == DEVICE) {
			(void)P::device_free(q);
		} else if (kind == PINNED) {
			(void)P::pinned_free(q);
		} else {
			(void)P::event_destroy(static_cast<event>(q));
		}
	}

	mutable std::mutex mu_;
	std::unordered_map<const void *, Kind> live_;
};
