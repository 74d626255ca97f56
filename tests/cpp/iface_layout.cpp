// iface_layout.cpp -- prints the layout of libadsb's listener / aircraft surface, one fact per line (tests/test_iface_matches_reference.py).
//
// Built as is, it describes the stand-alone slice in include/libadsb_iface.hpp.  Built with -DIFACE_LAYOUT_OF_REFERENCE and the reference
// checkout on the include path, it describes the reference's own ADSBListener.h and AircraftImpl.h (they need only CommonMacros.h, no
// <rtl-sdr.h>): that output is tests/golden/iface_reference_layout.txt, and `make -C oracle _ref/iface_layout REF=<checkout>` rebuilds it.
// The two outputs must be equal line for line: Source's underlying type and enumerators; every IAirCraft / IListener / IDataProvider member
// function with its signature and its virtual-table slot (which pins the order of the virtual functions); sizeof / alignof of every type;
// type and offsetof of every AirCraftImpl and TrafficManager data member; TrafficManager's member functions and its base.
//
// Types are spelled by name_of<> below rather than by the demangler, so the text does not depend on how a standard library spells
// std::chrono or std::unordered_map internally.  Virtual-table slots are read from pointers to member functions (Itanium C++ ABI: a virtual
// member's pointer holds 1 + its byte offset in the table).
#include <array>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <span>
#include <string>
#include <string_view>
#include <type_traits>
#include <unordered_map>

#ifdef IFACE_LAYOUT_OF_REFERENCE
namespace ref
{
#include "ADSBListener.h"
#include "AircraftImpl.h"
} // namespace ref
namespace side = ::ref::ADSB;
#else
#include "libadsb_iface.hpp" // stand-alone branch (LIBADSB_AMD_WITH_LIBADSB_HEADERS not defined)
namespace side = ::ADSB;
#endif

template <class T> struct name_of;
template <class T> std::string type_name() { return name_of<T>::get(); }

template <> struct name_of<void> { static std::string get() { return "void"; } };
template <> struct name_of<bool> { static std::string get() { return "bool"; } };
template <> struct name_of<char> { static std::string get() { return "char"; } };
template <> struct name_of<double> { static std::string get() { return "f64"; } };
template <> struct name_of<uint8_t> { static std::string get() { return "u8"; } };
template <> struct name_of<uint32_t> { static std::string get() { return "u32"; } };
template <> struct name_of<int32_t> { static std::string get() { return "i32"; } };
template <> struct name_of<std::string_view> { static std::string get() { return "string_view"; } };
template <> struct name_of<std::chrono::time_point<std::chrono::system_clock>> { static std::string get() { return "system_clock::time_point"; } };
template <> struct name_of<side::Source> { static std::string get() { return "Source"; } };
template <> struct name_of<side::IAirCraft> { static std::string get() { return "IAirCraft"; } };
template <> struct name_of<side::IListener> { static std::string get() { return "IListener"; } };
template <> struct name_of<side::IDataProvider> { static std::string get() { return "IDataProvider"; } };
template <> struct name_of<side::AirCraftImpl> { static std::string get() { return "AirCraftImpl"; } };
template <> struct name_of<side::TrafficManager> { static std::string get() { return "TrafficManager"; } };
template <class T> struct name_of<T const> { static std::string get() { return type_name<T>() + " const"; } };
template <class T> struct name_of<T&> { static std::string get() { return type_name<T>() + "&"; } };
template <class T> struct name_of<T*> { static std::string get() { return type_name<T>() + "*"; } };
template <class T, size_t N> struct name_of<std::array<T, N>> { static std::string get() { return "array<" + type_name<T>() + ", " + std::to_string(N) + ">"; } };
template <class T> struct name_of<std::unique_ptr<T>> { static std::string get() { return "unique_ptr<" + type_name<T>() + ">"; } };
template <class K, class V> struct name_of<std::unordered_map<K, V>>
{
    static std::string get() { return "unordered_map<" + type_name<K>() + ", " + type_name<V>() + ">"; }
};

template <class F> struct signature;
template <class C, class R, class... A> struct signature<R (C::*)(A...)>
{
    static std::string get() { return type_name<R>() + "(" + join<A...>() + ")"; }
    template <class... B> static std::string join()
    {
        std::string s;
        ((s += (s.empty() ? "" : ", ") + type_name<B>()), ...);
        return s;
    }
};
template <class C, class R, class... A> struct signature<R (C::*)(A...) const>
{
    static std::string get() { return signature<R (C::*)(A...)>::get() + " const"; }
};
template <class C, class R, class... A> struct signature<R (C::*)(A...) noexcept>
{
    static std::string get() { return signature<R (C::*)(A...)>::get() + " noexcept"; }
};
template <class C, class R, class... A> struct signature<R (C::*)(A...) const noexcept>
{
    static std::string get() { return signature<R (C::*)(A...)>::get() + " const noexcept"; }
};

// "slot=<n>" for a virtual member function, "non-virtual" otherwise
template <class F> std::string slot_of(F f)
{
    static_assert(sizeof(F) == 2 * sizeof(void*), "Itanium C++ ABI pointer to member function expected");
    uintptr_t word;
    std::memcpy(&word, &f, sizeof word);
    if ((word & 1u) == 0) return "non-virtual";
    return "slot=" + std::to_string((word - 1) / sizeof(void*));
}

template <class T> void type_line()
{
    std::printf("%s size=%zu align=%zu polymorphic=%d abstract=%d virtual_dtor=%d\n", type_name<T>().c_str(), sizeof(T), alignof(T),
                (int)std::is_polymorphic_v<T>, (int)std::is_abstract_v<T>, (int)std::has_virtual_destructor_v<T>);
}

#define MEMBER(Class, name) std::printf("%s::%s %s %s\n", #Class, #name, signature<decltype(&side::Class::name)>::get().c_str(), slot_of(&side::Class::name).c_str())
#define FIELD(Class, name) std::printf("%s::%s %s offset=%zu\n", #Class, #name, type_name<decltype(side::Class::name)>().c_str(), offsetof(side::Class, name))

int main()
{
    using S = side::Source;
    std::printf("Source underlying=%s UAT978=%u ADSB1090=%u FlightRadar24=%u\n", type_name<std::underlying_type_t<S>>().c_str(), (unsigned)S::UAT978,
                (unsigned)S::ADSB1090, (unsigned)S::FlightRadar24);

    type_line<side::IAirCraft>();
    std::printf("IAirCraft::time_point %s\n", type_name<side::IAirCraft::time_point>().c_str());
    MEMBER(IAirCraft, SourceId);
    MEMBER(IAirCraft, MessageCount);
    MEMBER(IAirCraft, Addr);
    MEMBER(IAirCraft, FlightNumber);
    MEMBER(IAirCraft, LastSeen);
    MEMBER(IAirCraft, SquakCode);
    MEMBER(IAirCraft, Altitude);
    MEMBER(IAirCraft, Speed);
    MEMBER(IAirCraft, Heading);
    MEMBER(IAirCraft, Climb);
    MEMBER(IAirCraft, Lat1E7);
    MEMBER(IAirCraft, Lon1E7);

    type_line<side::IListener>();
    MEMBER(IListener, OnChanged);
    MEMBER(IListener, OnDeviceStatusChanged);

    type_line<side::IDataProvider>();
    MEMBER(IDataProvider, Start);
    MEMBER(IDataProvider, Stop);
    MEMBER(IDataProvider, NotifySelfLocation);

    type_line<side::AirCraftImpl>();
    std::printf("AirCraftImpl derives from IAirCraft=%d\n", (int)std::is_base_of_v<side::IAirCraft, side::AirCraftImpl>);
    MEMBER(AirCraftImpl, SourceId);
    MEMBER(AirCraftImpl, Lon1E7);
    FIELD(AirCraftImpl, addr);
    FIELD(AirCraftImpl, callsign);
    FIELD(AirCraftImpl, seen);
    FIELD(AirCraftImpl, modeA);
    FIELD(AirCraftImpl, altitude);
    FIELD(AirCraftImpl, speed);
    FIELD(AirCraftImpl, track);
    FIELD(AirCraftImpl, vertRate);
    FIELD(AirCraftImpl, lat1E7);
    FIELD(AirCraftImpl, lon1E7);
    FIELD(AirCraftImpl, cprOddLat);
    FIELD(AirCraftImpl, cprOddLon);
    FIELD(AirCraftImpl, cprOddTime);
    FIELD(AirCraftImpl, cprEvenLat);
    FIELD(AirCraftImpl, cprEvenLon);
    FIELD(AirCraftImpl, cprEvenTime);
    FIELD(AirCraftImpl, sourceId);

    type_line<side::TrafficManager>();
    std::printf("TrafficManager derives from enable_shared_from_this<TrafficManager>=%d\n",
                (int)std::is_base_of_v<std::enable_shared_from_this<side::TrafficManager>, side::TrafficManager>);
    MEMBER(TrafficManager, FindOrCreate);
    MEMBER(TrafficManager, SetListener);
    MEMBER(TrafficManager, NotifyChanged);
    FIELD(TrafficManager, aircrafts);
    FIELD(TrafficManager, listener);
    return 0;
}
