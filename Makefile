# Builds the product library (HIP, gfx950) and the test-only oracle.
HIPCC ?= hipcc
ARCH ?= gfx950
HIPFLAGS = --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Iinclude
CSRC = ronkathon_amd/csrc
LIB = ronkathon_amd/libronk_ntt.so
OBJS = build/tile_kernels_wl.o build/tile_kernels_r4.o build/tile_kernels_mont.o build/tile_kernels_mont_feat.o build/tile_kernels_mont_mul.o build/tile_kernels.o build/tile_kernels_cfg.o build/tile_kernels_half.o build/tile_kernels_feat.o build/tile_kernels_mul.o build/tile_kernels_dist_mul.o build/small_kernels.o build/ronk_core.o build/ronk_plan.o build/ronk_callers.o build/ronk_workspace.o build/ronk_dist.o build/ronk_msm.o build/ronk_recover.o build/ronk_multipoint.o build/ronk_hash.o build/ronk_fr_ntt.o build/ronk_fri.o build/ronk_ext2.o build/ronk_pcs.o build/ronk_accum.o build/ronk_plonk.o build/ronk_pow.o build/ronk_lookup.o build/ronk_mpcs.o build/ronk_air.o build/ronk_stark.o
HDRS = $(wildcard $(CSRC)/*.h) $(wildcard include/*.h)

all: $(LIB) oracle
$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS)
build/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p build
	$(HIPCC) $(HIPFLAGS) -c $< -o $@
oracle:
	$(MAKE) -C oracle -s
clean:
	rm -rf build $(LIB)
	$(MAKE) -C oracle clean
.PHONY: all oracle clean

# Sanitizer builds of the host-side code: the oracle under ASan+UBSan, the field header and the
# tile kernel body + planner (the host emulator; Goldilocks and Montgomery field policies, the R4 round structure; the scan and long-division bodies, the Poseidon / sponge / Merkle bodies, the multipoint bodies, the BN254 scalar-field transform's pass body, the FRI fold / transcript / verifier bodies, the quadratic extension and the extension FRI bodies, the DEEP combination and extension-point evaluation bodies, the multi-matrix combination bodies, the scan and accumulator bodies, the PLONK quotient bodies, the proof-of-work bodies over the search kernel's grid, the lookup multiplicity bodies in three lane orders and the logUp quotient bodies, the constraint-program interpreter with and without periodic columns and the host construction of their tables, the STARK quotient split and transcript steps) under UBSan (ASan does not follow the emulator's ucontext fibers).
SAN = -g -O1 -fno-omit-frame-pointer -fno-sanitize-recover=all
sanitize:
	@mkdir -p build/san
	gcc $(SAN) -fsanitize=address,undefined -o build/san/oracle_san tests/emu/oracle_san.c oracle/ronk_oracle.c
	g++ $(SAN) -std=c++17 -fsanitize=address,undefined -o build/san/test_gl64_host tests/emu/test_gl64_host.cpp
	gcc -O1 -c -o build/san/orc.o oracle/ronk_oracle.c
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_tile tests/emu/emu_tile.cpp build/san/orc.o
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_scan tests/emu/emu_scan.cpp build/san/orc.o
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_longdiv tests/emu/emu_longdiv.cpp build/san/orc.o
	g++ $(SAN) -std=c++17 -fsanitize=address,undefined -o build/san/bn254_san tests/emu/bn254_san.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_poseidon tests/emu/emu_poseidon.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_multipoint tests/emu/emu_multipoint.cpp build/san/orc.o
	g++ $(SAN) -std=c++17 -fsanitize=undefined -pthread -o build/san/emu_fr_ntt tests/emu/emu_fr_ntt.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_fri tests/emu/emu_fri.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_ext2 tests/emu/emu_ext2.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_deep tests/emu/emu_deep.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_mpcs tests/emu/emu_mpcs.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_accum tests/emu/emu_accum.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_plonk tests/emu/emu_plonk.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_pow tests/emu/emu_pow.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_lookup tests/emu/emu_lookup.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_air tests/emu/emu_air.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_stark tests/emu/emu_stark.cpp
	g++ $(SAN) -std=c++17 -fsanitize=undefined -o build/san/emu_air_per tests/emu/emu_air_per.cpp
	./build/san/oracle_san
	./build/san/bn254_san
	./build/san/test_gl64_host
	./build/san/emu_tile 12 3 0 4 | tail -1
	./build/san/emu_tile 16 2 1 4 18 | tail -1
	./build/san/emu_tile 15 2 0 4 18 25 0 0 1 | tail -1
	./build/san/emu_tile 20 1 0 3 | tail -1
	./build/san/emu_tile dist 16 4 0 0 2 | tail -1
	./build/san/emu_tile mul 20 300001 7 2 18 | tail -1
	RONK_EMU_P=0xFFFFFFFC00000001 RONK_EMU_G=10 ./build/san/emu_tile 16 2 1 4 18 | tail -1
	RONK_EMU_P=0xc0000001 RONK_EMU_G=5 ./build/san/emu_tile 12 3 0 4 | tail -1
	RONK_R4MID=1 ./build/san/emu_tile 19 1 0 4 18 | tail -1
	./build/san/emu_tile 20 1 1 2 20 | tail -1
	RONK_WL_HALF=1 ./build/san/emu_tile 22 1 0 2 22 | tail -1
	RONK_EMU_P=0xFFFFFFFC00000001 RONK_EMU_G=10 ./build/san/emu_tile 20 1 0 2 18 | tail -1
	./build/san/emu_scan 18446744069414584321 70001 123456789 3 1 | tail -1
	./build/san/emu_scan 101 5000 7 3 0 | tail -1
	./build/san/emu_scan 18446744069414584321 70001 123456789 3 3 | tail -1
	EMU_LINDIV1_PL=4 ./build/san/emu_scan 18446744069414584321 30001 123456789 1 6 | tail -1
	./build/san/emu_scan 101 25000 7 3 2 | tail -1
	./build/san/emu_longdiv 18446744069414584321 120 300 64 3 | tail -1
	./build/san/emu_longdiv 101 120 300 64 3 | tail -1
	./build/san/emu_poseidon 18446744069414584321 12 7 22 8 8 1 | tail -1
	./build/san/emu_poseidon 0xFFFFFFFC00000001 16 5 3 5 15 2 | tail -1
	./build/san/emu_poseidon 101 3 11 2 3 2 3 | tail -1
	./build/san/emu_multipoint 197 397 7 1 | tail -1
	./build/san/emu_multipoint 197 196 7 0 | tail -1
	RONK_EMU_P=0xFFFFFFFC00000001 ./build/san/emu_multipoint 129 128 9 1 | tail -1
	RONK_EMU_P=101 ./build/san/emu_multipoint 50 103 3 1 | tail -1
	./build/san/emu_fr_ntt 9 5 3 7 | tail -1
	./build/san/emu_fr_ntt 12 4 1 7 | tail -1
	./build/san/emu_fri 18446744069414584321 7 | tail -1
	./build/san/emu_fri 0xFFFFFFFC00000001 10 | tail -1
	./build/san/emu_fri 0xC0000001 5 | tail -1
	./build/san/emu_ext2 18446744069414584321 7 | tail -1
	./build/san/emu_ext2 0xFFFFFFFC00000001 10 | tail -1
	./build/san/emu_ext2 0xC0000001 5 | tail -1
	./build/san/emu_ext2 18446744069414584321 11 | tail -1
	./build/san/emu_deep 18446744069414584321 7 | tail -1
	./build/san/emu_deep 18446744069414584321 7 11 | tail -1
	./build/san/emu_deep 0xFFFFFFFC00000001 10 | tail -1
	./build/san/emu_deep 0xC0000001 5 | tail -1
	./build/san/emu_mpcs 18446744069414584321 7 | tail -1
	./build/san/emu_mpcs 18446744069414584321 7 11 | tail -1
	./build/san/emu_mpcs 0xFFFFFFFC00000001 10 | tail -1
	./build/san/emu_mpcs 0xC0000001 5 | tail -1
	./build/san/emu_accum 18446744069414584321 7 | tail -1
	./build/san/emu_accum 18446744069414584321 11 | tail -1
	./build/san/emu_accum 0xFFFFFFFC00000001 10 | tail -1
	./build/san/emu_accum 17 3 | tail -1
	./build/san/emu_plonk 18446744069414584321 7 7 9 2 7 1 | tail -1
	./build/san/emu_plonk 18446744069414584321 7 11 10 3 7 0 | tail -1
	./build/san/emu_plonk 0xFFFFFFFC00000001 10 10 11 1 10 1 | tail -1
	./build/san/emu_plonk 97 5 5 1 1 5 1 | tail -1
	./build/san/emu_pow 18446744069414584321 8 7 2 4 4 10 16 512 11 22 33 44 55 | tail -1
	./build/san/emu_pow 0xFFFFFFFC00000001 12 7 22 8 8 6 12 64 1 2 3 4 5 6 7 8 | tail -1
	./build/san/emu_pow 0xC000002400000001 16 7 2 4 15 10 4 64 9 | tail -1
	./build/san/emu_pow 101 3 5 2 4 2 3 6 16 100 7 | tail -1
	./build/san/emu_lookup 18446744069414584321 7 7 | tail -1
	./build/san/emu_lookup 0xFFFFFFFC00000001 10 10 | tail -1
	./build/san/emu_lookup 17 3 3 | tail -1
	./build/san/emu_air 18446744069414584321 7 7 | tail -1
	./build/san/emu_air 18446744069414584321 7 11 | tail -1
	./build/san/emu_air 0xFFFFFFFC00000001 10 10 | tail -1
	./build/san/emu_air 17 3 3 | tail -1
	./build/san/emu_stark 18446744069414584321 7 | tail -1
	./build/san/emu_stark 18446744069414584321 11 | tail -1
	./build/san/emu_stark 0xFFFFFFFC00000001 10 | tail -1
	./build/san/emu_stark 97 5 | tail -1
	./build/san/emu_stark 17 3 | tail -1
	./build/san/emu_air_per 18446744069414584321 7 7 | tail -1
	./build/san/emu_air_per 18446744069414584321 7 11 | tail -1
	./build/san/emu_air_per 0xFFFFFFFC00000001 10 10 | tail -1
	./build/san/emu_air_per 97 5 5 | tail -1
	./build/san/emu_air_per 17 3 3 | tail -1
	# the emulators' directed mode (emu_ref.h): small signed words, which take the ">= p" outcomes of gl64.h all the time
	RONK_EMU_SMALL=2 ./build/san/emu_poseidon 18446744069414584321 12 1 22 8 8 1 | tail -1
	RONK_EMU_SMALL=2 ./build/san/emu_fri 18446744069414584321 7 | tail -1
	RONK_EMU_SMALL=8 ./build/san/emu_ext2 18446744069414584321 7 | tail -1
	RONK_EMU_SMALL=2 ./build/san/emu_deep 18446744069414584321 7 11 | tail -1
	RONK_EMU_SMALL=2 ./build/san/emu_mpcs 18446744069414584321 7 | tail -1
	RONK_EMU_SMALL=2 ./build/san/emu_accum 18446744069414584321 7 | tail -1
	RONK_EMU_SMALL=2 ./build/san/emu_plonk 18446744069414584321 7 7 4 2 7 1 | tail -1
	RONK_EMU_SMALL=2 ./build/san/emu_air 18446744069414584321 7 7 | tail -1
	RONK_EMU_SMALL=2 ./build/san/emu_air_per 18446744069414584321 7 7 | tail -1
.PHONY: sanitize
