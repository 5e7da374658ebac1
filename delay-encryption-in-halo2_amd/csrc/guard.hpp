// guard.hpp -- the one place where a C entry point's exceptions become return codes (include/dehalo.h: "never aborts, never throws").
// Host-only and free of HIP headers: witness.hip is also built by g++ alone (make host_sanitize / host_tsan).
#pragma once
#include <cstddef>
#include <exception>
#include <new>

#include "../../include/dehalo.h"

// body() or, when it throws: std::bad_alloc -> DEHALO_ERR_OOM; any other exception -> DEHALO_ERR_INVALID, its message handed to note(const char*)
// (a context's last error).  A note that throws in turn loses only its message.
template <class Note, class Body>
int dh_guard_noting(Note&& note, Body&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return DEHALO_ERR_OOM;
    } catch (const std::exception& e) {
        try { note(e.what()); } catch (...) {}
    } catch (...) {
        try { note("unexpected exception"); } catch (...) {}
    }
    return DEHALO_ERR_INVALID;
}

// an entry point with no context in reach (transcript, field info, witness synthesis): the message is dropped
template <class Body>
int dh_guard(std::nullptr_t, Body&& body) noexcept {
    return dh_guard_noting([](const char*) {}, body);
}
