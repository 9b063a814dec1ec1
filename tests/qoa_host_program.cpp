// Stand-alone host program over csrc/gas_qoa.h for tests/test_qoa_host_program.py, built with plain g++ under
// -fsanitize=address,undefined.
//   qoa_host_program deq                        prints the dequantisation table, 8 values per line
//   qoa_host_program FILE CHANNELS FRAMES       validates the file; "refused" and exit status 2 if it is none of a
//       stream of CHANNELS x FRAMES; else builds the records and prints one line "R h0 h1 h2 h3 w0 w1 w2 w3" per chunk
//       and channel, then one line per frame with the per-load decode (gas_qoa_record_sample) of every channel.
// The file is read into a heap block of exactly its size, so a read past its end is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gas_qoa.h"

int main(int argc, char **argv) {
	if (argc == 2 && std::strcmp(argv[1], "deq") == 0) {
		for (uint32_t i = 0; i < GAS_QOA_DEQ_ENTRIES; i++) {
			std::printf("%d%c", gas_qoa_dequant(i), i % 8 == 7 ? '\n' : ' ');
		}
		return 0;
	}
	if (argc != 4) {
		return 1;
	}
	std::FILE *fp = std::fopen(argv[1], "rb");
	if (!fp) {
		return 1;
	}
	std::fseek(fp, 0, SEEK_END);
	const long size = std::ftell(fp);
	std::fseek(fp, 0, SEEK_SET);
	uint8_t *data = static_cast<uint8_t *>(std::malloc(size > 0 ? (size_t)size : 1));
	if (!data || std::fread(data, 1, (size_t)size, fp) != (size_t)size) {
		return 1;
	}
	std::fclose(fp);
	const uint32_t channels = (uint32_t)std::strtoul(argv[2], nullptr, 10);
	const uint64_t frames = std::strtoull(argv[3], nullptr, 10);
	if (!gas_qoa_validate(data, (uint64_t)size, channels, frames)) {
		std::puts("refused");
		std::free(data);
		return 2;
	}
	std::vector<gas_qoa_record> recs(gas_qoa_chunks(frames) * channels, gas_qoa_record{});
	gas_qoa_build_records(data, channels, frames, recs.data());
	std::free(data);
	for (const gas_qoa_record &r : recs) {
		std::printf("R %d %d %d %d %d %d %d %d\n", r.history[0], r.history[1], r.history[2], r.history[3], r.weights[0], r.weights[1], r.weights[2], r.weights[3]);
	}
	for (uint64_t i = 0; i < frames; i++) {
		for (uint32_t c = 0; c < channels; c++) {
			std::printf("%d%c", gas_qoa_record_sample(recs[(i / GAS_QOA_CHUNK) * channels + c], (uint32_t)(i % GAS_QOA_CHUNK)), c + 1 == channels ? '\n' : ' ');
		}
	}
	return 0;
}
