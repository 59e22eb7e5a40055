// mesh_light_state_cpu.cpp -- MeshLightState (csrc/flx_feature_state.h) without a GPU: reads one sequence of events per line from stdin and prints
// the state's queries after the last one.  Events: on off wf_on wf_off upload:<lights> moved rebuilt.  tests/test_mesh_light_state.py drives it.
#include "../fluctus_amd/csrc/flx_feature_state.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        flxd::MeshLightState s;
        std::istringstream in(line);
        std::string ev;
        while (in >> ev) {
            if (ev == "on") s.optionSet(true);
            else if (ev == "off") s.optionSet(false);
            else if (ev == "wf_on") s.wavefrontSet(true);
            else if (ev == "wf_off") s.wavefrontSet(false);
            else if (ev.rfind("upload:", 0) == 0) s.sceneUploaded((uint32_t)std::strtoul(ev.c_str() + 7, nullptr, 10));
            else if (ev == "moved") s.trianglesMoved();
            else if (ev == "rebuilt") s.rebuilt();
            else { std::fprintf(stderr, "unknown event %s\n", ev.c_str()); return 2; }
            if (s.needsBuild()) s.rebuilt();           // meshLightsSync at the end of every call: never stale with the option on
        }
        std::printf("%d %d %d %d %d\n", (int)s.on, (int)s.wavefront, (int)s.usable(), (int)s.lit(), (int)s.litWavefront());
    }
    return 0;
}
