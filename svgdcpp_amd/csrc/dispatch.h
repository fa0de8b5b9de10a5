// dispatch.h -- a run-time value to a compile-time constant (internal).
//
// dispatch<LIST>(v, f) walks the constexpr array LIST (built.h) and calls the
// generic lambda f with std::integral_constant<int, LIST[i]> for the entry
// equal to v; a list of TileClass takes (KP, NCB) and passes two constants;
// dispatch_range<LO, HI> is the list LO .. HI.  The lambda's body is instantiated once per entry, so the kernels it names
// are built for exactly the list.  Returns false when v is not in the list
// (the launcher then answers hipErrorInvalidValue) or when f itself returns
// false (a nested dispatch that found nothing).
#pragma once
#include <stddef.h>

#include <iterator>
#include <type_traits>
#include <utility>

#include "built.h"

namespace svgd_amd {
namespace detail {

template <class F, class... C> bool dispatch_call(F &f, C... c)
{
    if constexpr (std::is_void_v<decltype(f(c...))>) {
        f(c...);
        return true;
    } else {
        return f(c...);
    }
}

template <auto &LIST, class F, size_t... I> bool dispatch_int(int v, F &f, std::index_sequence<I...>)
{
    return ((v == LIST[I] && dispatch_call(f, std::integral_constant<int, LIST[I]>{})) || ...);
}

template <auto &LIST, class F, size_t... I> bool dispatch_tile(TileClass t, F &f, std::index_sequence<I...>)
{
    return ((t == LIST[I] && dispatch_call(f, std::integral_constant<int, LIST[I].KP>{},
                                           std::integral_constant<int, LIST[I].NCB>{})) ||
            ...);
}

template <int LO, class F, size_t... I> bool dispatch_range(int v, F &f, std::index_sequence<I...>)
{
    return ((v == LO + (int)I && dispatch_call(f, std::integral_constant<int, LO + (int)I>{})) || ...);
}

} // namespace detail

// the list LO .. HI (kernels no plan chooses between: one per dimension)
template <int LO, int HI, class F> bool dispatch_range(int v, F &&f)
{
    return detail::dispatch_range<LO>(v, f, std::make_index_sequence<HI - LO + 1>{});
}

template <auto &LIST, class F> bool dispatch(int v, F &&f)
{
    return detail::dispatch_int<LIST>(v, f, std::make_index_sequence<std::size(LIST)>{});
}

template <auto &LIST, class F> bool dispatch(int KP, int NCB, F &&f)
{
    return detail::dispatch_tile<LIST>(TileClass{KP, NCB}, f, std::make_index_sequence<std::size(LIST)>{});
}

} // namespace svgd_amd
