# Convenience targets; `python -m kasa_amd.build` and `__graft_entry__.build()` do the same compiles.
HIPCC ?= /opt/rocm/bin/hipcc
LIB    = kasa_amd/libkasa_hip.so
HOST   = kasa_amd/host/kasa_identify
INDEX  = kasa_amd/host/kasa_index

all: $(LIB) $(HOST) $(INDEX) oracle

$(LIB): kasa_amd/csrc/kasa_hip.hip kasa_amd/csrc/kasa_refbatch.cpp kasa_amd/csrc/stdsort_order.h kasa_amd/csrc/kasa_radix.h kasa_amd/csrc/kasa_text.h kasa_amd/csrc/kasa_replay.h kasa_amd/csrc/kasa_build.h kasa_amd/csrc/kasa_edit.h kasa_amd/csrc/kasa_spill.h kasa_amd/csrc/kasa_spill_plan.h kasa_amd/csrc/kasa_parse.h kasa_amd/csrc/kasa_bgzf.h kasa_amd/csrc/kasa_inflate.h kasa_amd/csrc/kasa_gunzip.h kasa_amd/host/grisu_powers.inc include/kasa_hip.h
	$(HIPCC) --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off -Wall -Wno-unused-result -o $@ kasa_amd/csrc/kasa_hip.hip kasa_amd/csrc/kasa_refbatch.cpp -ldl -Wl,-rpath,/opt/rocm/lib

$(HOST): kasa_amd/host/kasa_identify.cpp kasa_amd/host/grisu_powers.inc include/kasa_hip.h $(LIB)
	g++ -O2 -std=c++17 -pthread -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -o $@ $< -Lkasa_amd -lkasa_hip -lz -L/opt/rocm/lib -lrccl -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib

# merge | redundancy | trie: the same source with -DKASA_INDEX_TOOL
$(INDEX): kasa_amd/host/kasa_identify.cpp kasa_amd/host/grisu_powers.inc include/kasa_hip.h $(LIB)
	g++ -O2 -std=c++17 -pthread -DKASA_INDEX_TOOL -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -o $@ $< -Lkasa_amd -lkasa_hip -lz -L/opt/rocm/lib -lrccl -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib

oracle:
	$(MAKE) -C oracle

# host code under AddressSanitizer + UBSan (device code objects unchanged: -fno-gpu-sanitize); run with tools/asan_run.sh
ASAN_RT = $(shell /opt/rocm/lib/llvm/bin/clang --print-file-name=libclang_rt.asan-x86_64.so)
asan: kasa_amd/libkasa_hip_asan.so kasa_amd/host/kasa_identify_asan
kasa_amd/libkasa_hip_asan.so: kasa_amd/csrc/kasa_hip.hip kasa_amd/csrc/kasa_refbatch.cpp kasa_amd/csrc/stdsort_order.h kasa_amd/csrc/kasa_radix.h kasa_amd/csrc/kasa_text.h kasa_amd/csrc/kasa_replay.h include/kasa_hip.h
	$(HIPCC) --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -shared -ffp-contract=off -fsanitize=address,undefined -fno-gpu-sanitize -shared-libsan -fno-omit-frame-pointer -Wno-unused-result -o $@ kasa_amd/csrc/kasa_hip.hip kasa_amd/csrc/kasa_refbatch.cpp -ldl -Wl,-rpath,/opt/rocm/lib -Wl,-rpath,$(dir $(ASAN_RT))
kasa_amd/host/kasa_identify_asan: kasa_amd/host/kasa_identify.cpp kasa_amd/host/grisu_powers.inc include/kasa_hip.h kasa_amd/libkasa_hip_asan.so
	/opt/rocm/lib/llvm/bin/clang++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -shared-libsan -fno-omit-frame-pointer -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -o $@ $< kasa_amd/libkasa_hip_asan.so -lz -L/opt/rocm/lib -lrccl -Wl,-rpath,'$$ORIGIN/..' -Wl,-rpath,/opt/rocm/lib -Wl,-rpath,$(dir $(ASAN_RT))

# the decoder body of kasa_inflate.h for the CPU under AddressSanitizer + UBSan: a stand-alone program, run as
#   tools/inflate_host_check DIR    (DIR: NAME.bgzf with NAME.raw or NAME.status; tests/test_inflate_cpu.py writes one)
tools/inflate_host_check: tools/inflate_host_check.cpp kasa_amd/csrc/kasa_inflate.h include/kasa_hip.h
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -o $@ $<

# the bodies and the rounds of kasa_gunzip.h likewise:
#   tools/gunzip_host_check DIR [chunkBytes ...]    (DIR: NAME.gz with NAME.raw or NAME.status; tests/test_gzip_corpus_cpu.py writes one)
tools/gunzip_host_check: tools/gunzip_host_check.cpp kasa_amd/csrc/kasa_gunzip.h kasa_amd/csrc/kasa_inflate.h include/kasa_hip.h
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -o $@ $<

# the slab plan of kasa_spill_plan.h (builds larger than device memory) likewise:
#   tools/spill_plan_check FILE ...    (FILE: "letters budget runs", then per run its length and its keys; tests/test_spill_cpu.py writes them)
tools/spill_plan_check: tools/spill_plan_check.cpp kasa_amd/csrc/kasa_spill_plan.h
	g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -fno-omit-frame-pointer -pthread -o $@ $<

test:
	python -m pytest tests -q -m "not gpu"

test-gpu:
	python -m pytest tests -q -m gpu

clean:
	rm -f $(LIB) $(HOST) $(INDEX) kasa_amd/libkasa_hip_asan.so kasa_amd/host/kasa_identify_asan tools/inflate_host_check tools/gunzip_host_check tools/spill_plan_check
	$(MAKE) -C oracle clean

.PHONY: all oracle test test-gpu clean asan
