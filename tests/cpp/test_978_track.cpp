// test_978_track.cpp -- the reference's UAT flow for a host WITHOUT dump978's decoder: this binary defines no
// dump_raw_message, so the GPU handler (ADSB::test::TryCreateUAT978Handler) tracks aircraft itself and calls the traffic
// manager's listener once per frame.  The listener prints each OnChanged as the reference's test listener formats it
// (tests/test_1090.cpp:19-28: "{:x}[{: >8}]: Pos={:+03.2f}:{:+03.2f}^{:05} Speed={:03} Count={}", the call sign's eight raw
// bytes included).   usage: test_978_track <iq file> <bytes per HandleData call>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "libadsb_iface.hpp"

struct Listener : ADSB::IListener
{
    void OnChanged(ADSB::IAirCraft const& a) override
    {
        const std::string_view cs = a.FlightNumber();
        std::printf("%x[", a.Addr());
        for (size_t i = cs.size(); i < 8; i++) std::fputc(' ', stdout);
        std::fwrite(cs.data(), 1, cs.size(), stdout);
        std::printf("]: Pos=%+03.2f:%+03.2f^%05d Speed=%03u Count=%u\n", a.Lat1E7() / 10000000., a.Lon1E7() / 10000000., a.Altitude(), a.Speed(),
                    a.SquakCode());
        if (a.SourceId() != ADSB::Source::UAT978) std::printf("!! source id\n");
    }
    void OnDeviceStatusChanged(ADSB::Source, bool) override {}
};

struct Selector : RTLSDR::IDeviceSelector
{
    [[nodiscard]] bool SelectDevice(RTLSDR::DeviceInfo const&) const override { return false; }
};

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    std::ifstream        f(argv[1], std::ios::binary);
    std::vector<uint8_t> iq((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const size_t         step = std::strtoull(argv[2], nullptr, 10);
    auto                 mgr  = std::make_shared<ADSB::TrafficManager>();
    Listener             listener;
    mgr->SetListener(&listener);
    Selector selector;
    auto     handler = ADSB::test::TryCreateUAT978Handler(mgr, &selector, ADSB::Source::UAT978);
    for (size_t o = 0; o < iq.size(); o += step) handler->HandleData({iq.data() + o, std::min(step, iq.size() - o)});
    return 0;
}
