// Stand-alone host program over csrc/gas_switches.h for tests/test_switches_host_program.py, built with plain g++ under
// -fsanitize=address,undefined.
//   switches_host_program                  fills a gas_switches from the environment and prints it, "field=value ..."
//   switches_host_program NAME VALUE       the same, then setenv(NAME, VALUE) ("-": unsetenv), a second fill and a
//                                          second line: the reader is a function of the environment, not a static
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gas_switches.h"

static void print(const gas_switches &s) {
	std::printf("rows_first=%d adpcm_span=%d qoa_span=%d uni_flt=%d uni_er_mode=%d xcd_order_auto_min=%u shelf_scan=%d biquad_pipe=%d\n", (int)s.rows_first, (int)s.adpcm_span, (int)s.qoa_span, (int)s.uni_flt, s.uni_er_mode, (unsigned)s.xcd_order_auto_min, (int)s.shelf_scan, (int)s.biquad_pipe);
}

int main(int argc, char **argv) {
	if (argc != 1 && argc != 3) {
		return 1;
	}
	print(gas_switches_from_env());
	if (argc == 3) {
		if (std::strcmp(argv[2], "-") == 0 ? unsetenv(argv[1]) : setenv(argv[1], argv[2], 1)) {
			return 1;
		}
		print(gas_switches_from_env());
	}
	return 0;
}
