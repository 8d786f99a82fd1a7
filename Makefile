# Builds (for gfx950):
#   hartallo_amd/libhartallo_amd.so  the product: HIP kernels (k_pipeline in three builds) + host writer + C ABI
#   tests/emu/libhl_emu.so           test-only host build of the kernel logic
#   tests/emu/libhl_pyr_emu.so       test-only host build of the layer pyramid (hl_pyramid.h)
#   tests/emu/libhl_scene_emu.so     test-only host build of the scene-cut analysis (hl_scene.h)
#   tests/emu/libhl_quality_emu.so   test-only host build of the quality metric (hl_quality.h)
#   tests/emu/libhl_ingest_emu.so    test-only host build of the frame ingest (hl_ingest.h)
#   tests/emu/libhl_display_emu.so   test-only host build of the display size's edge tiles and quality window (hl_ingest.h, hl_quality.h)
#   tests/emu/libhl_scale_emu.so     test-only host build of the area downscaler behind the ingest (hl_scale.h, hl_ingest.h)
#   tests/emu/libhl_ladder_emu.so    test-only host build of the rendition ladder's fan-out behind one ingest (hl_ladder.h, hl_ingest.h)
#   tests/emu/libhl_svc_display_emu.so  test-only host build of the ingest's edge tiles with margins wider than a macroblock (hl_ingest.h)
#   tests/emu/libhl_svc_geom_emu.so  test-only host exports of the enhancement layers' constants and Intra_Base sample (hl_svc.h)
#   tests/emu/libhl_sched_emu.so     test-only host build of the pipelined run's pop (hl_sched.h)
#   tests/emu/libhl_rec_emu.so       test-only host exports of the candidate record's pack / unpack (hl_mbcore.h)
#   tests/gpu_unit/libhl_unit.so     test-only GPU unit kernels (coop pipeline vs scalar primitives)
#   tests/gpu_unit/libhl_unit_cand.so  test-only GPU unit kernel (the search's candidate slot)
#   tests/gpu_unit/libhl_unit_rec.so   test-only GPU unit kernel (the search's candidate record and selection)
#   oracle/...                       test-only CPU oracle and reference build (oracle/Makefile)
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CSRC    := hartallo_amd/csrc
REF     ?= /root/reference
HDRS    := $(wildcard $(CSRC)/*.h) include/hartallo_amd.h
HOSTSRC := $(CSRC)/hl_writer.cpp $(CSRC)/hl_rc.cpp
# the product kernels, k_pipeline again with the 8x8-family helpers (runs of one picture)
# and once more with 256-lane workgroups (two macroblocks per CU)
KSRC    := $(CSRC)/hl_encoder.hip $(CSRC)/hl_encoder_fam3.hip $(CSRC)/hl_encoder_t256.hip
# -ffp-contract=off: the RDO costs are IEEE double and must round exactly like the reference
CXXFLAGS := -std=c++17 -O3 -fPIC -ffp-contract=off -Wall -Wno-unused-function -Wno-unused-variable
# device code scheduling of the product: the ILP-iterative strategy shortens
# the latency-bound macroblock decision (1088p bench +1.5 %, bit-exact;
# profiles/r02_sched_strategy_ab.log)
DEVFLAGS := -mllvm -amdgpu-sched-strategy=iterative-ilp
# k_ingest (hl_ingest.hip) is compiled on its own, without DEVFLAGS: that
# strategy crashes the compiler's register allocator on the planar-RGB kernel
# k_scale (hl_scale.hip) and k_scale_fan (hl_ladder.hip) likewise: bandwidth-bound, nothing to gain from that strategy
INGOBJ  := build/obj/hl_ingest.o build/obj/hl_scale.o build/obj/hl_ladder.o

.PHONY: all product emu unit oracle profile poison variant sanitize ubsan clean
all: product emu unit oracle sanitize

product: hartallo_amd/libhartallo_amd.so
emu: tests/emu/libhl_emu.so tests/emu/libhl_pyr_emu.so tests/emu/libhl_scene_emu.so tests/emu/libhl_quality_emu.so tests/emu/libhl_ingest_emu.so tests/emu/libhl_display_emu.so tests/emu/libhl_scale_emu.so tests/emu/libhl_ladder_emu.so tests/emu/libhl_svc_display_emu.so tests/emu/libhl_svc_geom_emu.so tests/emu/libhl_rec_emu.so tests/emu/libhl_sched_emu.so
unit: tests/gpu_unit/libhl_unit.so tests/gpu_unit/libhl_unit_cand.so tests/gpu_unit/libhl_unit_rec.so

build/obj/hl_ingest.o: $(CSRC)/hl_ingest.hip $(CSRC)/hl_ingest.h
	mkdir -p build/obj
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -c -o $@ $(CSRC)/hl_ingest.hip

build/obj/hl_scale.o: $(CSRC)/hl_scale.hip $(CSRC)/hl_scale.h
	mkdir -p build/obj
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -c -o $@ $(CSRC)/hl_scale.hip

build/obj/hl_ladder.o: $(CSRC)/hl_ladder.hip $(CSRC)/hl_ladder.h $(CSRC)/hl_scale.h
	mkdir -p build/obj
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -c -o $@ $(CSRC)/hl_ladder.hip

hartallo_amd/libhartallo_amd.so: $(KSRC) $(HOSTSRC) $(HDRS) $(INGOBJ)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) $(DEVFLAGS) -shared -o $@ $(KSRC) $(HOSTSRC) -x none $(INGOBJ)

# (hl_emu_search.hip = hl_emu_ctl.hip plus the search table's export;
# hl_emu_ctl.hip = hl_emu_memo.hip plus emu_encode_frame_ex; hl_emu_memo.hip =
# hl_emu.hip plus the memo's settings, counters and key export)
EMUSRC := tests/emu/hl_emu_search.hip
EMUINC := tests/emu/hl_emu_ctl.hip tests/emu/hl_emu_memo.hip tests/emu/hl_emu.hip
tests/emu/libhl_emu.so: $(EMUSRC) $(EMUINC) $(HOSTSRC) $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -O2 -DHL_FAM3=1 -shared -o $@ $(EMUSRC) $(HOSTSRC)

# the layer pyramid's per-span code on the host (no device code: a plain C++ source for the host compiler)
tests/emu/libhl_pyr_emu.so: tests/emu/hl_pyr_emu.cpp $(CSRC)/hl_pyramid.h
	$(CXX) -std=c++17 -O2 -fPIC -Wall -shared -o $@ tests/emu/hl_pyr_emu.cpp

# the scene-cut analysis' staging and per-macroblock code on the host (no device code)
tests/emu/libhl_scene_emu.so: tests/emu/hl_scene_emu.cpp $(CSRC)/hl_scene.h
	$(CXX) -std=c++17 -O2 -fPIC -Wall -shared -o $@ tests/emu/hl_scene_emu.cpp

# the quality metric's staging, per-strip and per-window code on the host (no device code)
tests/emu/libhl_quality_emu.so: tests/emu/hl_quality_emu.cpp $(CSRC)/hl_quality.h
	$(CXX) -std=c++17 -O2 -fPIC -Wall -shared -o $@ tests/emu/hl_quality_emu.cpp

# the frame ingest's per-tile code on the host (no device code)
tests/emu/libhl_ingest_emu.so: tests/emu/hl_ingest_emu.cpp $(CSRC)/hl_ingest.h
	$(CXX) -std=c++17 -O2 -fPIC -Wall -shared -o $@ tests/emu/hl_ingest_emu.cpp

# a display size below the coded size on the host: the ingest's full and edge tiles, the quality metric's window (no device code)
tests/emu/libhl_display_emu.so: tests/emu/hl_display_emu.cpp $(CSRC)/hl_ingest.h $(CSRC)/hl_quality.h
	$(CXX) -std=c++17 -O2 -fPIC -Wall -shared -o $@ tests/emu/hl_display_emu.cpp

# the area downscaler behind the ingest on the host: k_scale's per-lane functions looped over a frame (no device code)
tests/emu/libhl_scale_emu.so: tests/emu/hl_scale_emu.cpp $(CSRC)/hl_scale.h $(CSRC)/hl_ingest.h
	$(CXX) -std=c++17 -O2 -fPIC -Wall -shared -o $@ tests/emu/hl_scale_emu.cpp

# the rendition ladder on the host: one ingest at the source size, then k_scale_fan's block selection and per-lane functions looped over a launch (no device code)
tests/emu/libhl_ladder_emu.so: tests/emu/hl_ladder_emu.cpp $(CSRC)/hl_ladder.h $(CSRC)/hl_scale.h $(CSRC)/hl_ingest.h
	$(CXX) -std=c++17 -O2 -fPIC -Wall -shared -o $@ tests/emu/hl_ladder_emu.cpp

# the access unit's display size on the host: the ingest's tiles with margins up to (16 << K) - 2 (no device code)
tests/emu/libhl_svc_display_emu.so: tests/emu/hl_svc_display_emu.cpp $(CSRC)/hl_ingest.h
	$(CXX) -std=c++17 -O2 -fPIC -Wall -shared -o $@ tests/emu/hl_svc_display_emu.cpp

# the enhancement layers' per-layer constants and Intra_Base luma sample on the host (hl_filters.h brings its kernels along, as in libhl_emu.so)
tests/emu/libhl_svc_geom_emu.so: tests/emu/hl_svc_geom_emu.hip $(CSRC)/hl_writer.cpp $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -O2 -shared -o $@ tests/emu/hl_svc_geom_emu.hip $(CSRC)/hl_writer.cpp

# the pop's key, choice, head rule and slot / claim transitions on the host (no device code)
tests/emu/libhl_sched_emu.so: tests/emu/hl_sched_emu.cpp $(CSRC)/hl_sched.h
	$(CXX) -std=c++17 -O2 -fPIC -Wall -shared -o $@ tests/emu/hl_sched_emu.cpp

# the candidate record's pack and unpack functions on the host (no device code)
tests/emu/libhl_rec_emu.so: tests/emu/hl_rec_emu.hip $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -O2 --cuda-host-only -shared -o $@ tests/emu/hl_rec_emu.hip

tests/gpu_unit/libhl_unit.so: tests/gpu_unit/hl_unit.hip $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -shared -o $@ tests/gpu_unit/hl_unit.hip

tests/gpu_unit/libhl_unit_cand.so: tests/gpu_unit/hl_unit_cand.hip $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -shared -o $@ tests/gpu_unit/hl_unit_cand.hip

tests/gpu_unit/libhl_unit_rec.so: tests/gpu_unit/hl_unit_rec.hip $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) -shared -o $@ tests/gpu_unit/hl_unit_rec.hip

# sanitizer builds of the host code (tests/test_sanitizers.py, CPU):
#   tests/sanitize/libhl_emu_asan.so  the emulator (the kernel logic on the
#       host) under AddressSanitizer, the product's host writer (hl_writer.cpp)
#       and rate controller (hl_rc.cpp) under AddressSanitizer +
#       UndefinedBehaviorSanitizer; run with the clang ASan runtime preloaded
#   tests/sanitize/rowgate_tsan  the pipelined run's row-gated slice writers
#       (hl_writer.h RowGate) under ThreadSanitizer
#   tests/sanitize/pop_tsan  the pipelined run's pop protocol (hl_sched.h with
#       task_deps / task_succ) on 16 threads under ThreadSanitizer
#   tests/sanitize/ingest_asan  the frame ingest's per-tile code (hl_ingest.h)
#       over exactly-sized heap buffers under AddressSanitizer +
#       UndefinedBehaviorSanitizer (plain C++; like the two above, the
#       program carries the sanitizers' runtimes itself)
#   tests/sanitize/ingest_edge_asan  the same for frames of a display size below
#       the coded size: the full tiles and the edge tiles (in_tile_edge)
#   tests/sanitize/ingest_wide_asan  the same for the top layer of an encoder
#       with spatial layers: margins up to (16 << K) - 2, several edge tile columns
#   tests/sanitize/scale_asan  the area downscaler behind the ingest (hl_scale.h):
#       exactly-sized source planes, every output sample against a scalar
#       statement of the definition
#   tests/sanitize/ladder_asan  the rendition ladder's fan-out (hl_ladder.h): the
#       same for every rung of a launch, the LDS image sized for the launch's maximum
# (hipcc: every -fsanitize= directly after -Xarch_host, host code only)
SANFLAGS := -std=c++17 -O1 -g -fno-omit-frame-pointer -fPIC -ffp-contract=off -Wno-unused-function -Wno-unused-variable
ASAN := -Xarch_host -fsanitize=address
UBSAN := -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined
sanitize: tests/sanitize/libhl_emu_asan.so tests/sanitize/rowgate_tsan tests/sanitize/pop_tsan tests/sanitize/ingest_asan tests/sanitize/ingest_edge_asan tests/sanitize/ingest_wide_asan tests/sanitize/scale_asan tests/sanitize/ladder_asan
tests/sanitize/hl_writer_asan.o: $(CSRC)/hl_writer.cpp $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(SANFLAGS) $(ASAN) $(UBSAN) -c -o $@ $<
tests/sanitize/hl_rc_asan.o: $(CSRC)/hl_rc.cpp $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(SANFLAGS) $(ASAN) $(UBSAN) -c -o $@ $<
tests/sanitize/hl_emu_asan.o: $(EMUSRC) $(EMUINC) $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(SANFLAGS) -DHL_FAM3=1 $(ASAN) -c -o $@ $<
tests/sanitize/libhl_emu_asan.so: tests/sanitize/hl_emu_asan.o tests/sanitize/hl_writer_asan.o tests/sanitize/hl_rc_asan.o
	$(HIPCC) --offload-arch=$(ARCH) $(ASAN) $(UBSAN) -shared-libsan -shared -o $@ $^
tests/sanitize/rowgate_tsan: tests/sanitize/rowgate_tsan.cpp $(CSRC)/hl_writer.cpp $(HDRS)
	$(HIPCC) $(SANFLAGS) -Xarch_host -fsanitize=thread -o $@ tests/sanitize/rowgate_tsan.cpp $(CSRC)/hl_writer.cpp -lpthread
tests/sanitize/pop_tsan: tests/sanitize/pop_tsan.cpp $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(SANFLAGS) -Xarch_host -fsanitize=thread -o $@ -x hip tests/sanitize/pop_tsan.cpp -lpthread
tests/sanitize/ingest_asan: tests/sanitize/ingest_asan.cpp $(CSRC)/hl_ingest.h
	$(HIPCC) $(SANFLAGS) $(ASAN) $(UBSAN) -o $@ -x c++ tests/sanitize/ingest_asan.cpp
tests/sanitize/ingest_edge_asan: tests/sanitize/ingest_edge_asan.cpp $(CSRC)/hl_ingest.h
	$(HIPCC) $(SANFLAGS) $(ASAN) $(UBSAN) -o $@ -x c++ tests/sanitize/ingest_edge_asan.cpp
tests/sanitize/ingest_wide_asan: tests/sanitize/ingest_wide_asan.cpp $(CSRC)/hl_ingest.h
	$(HIPCC) $(SANFLAGS) $(ASAN) $(UBSAN) -o $@ -x c++ tests/sanitize/ingest_wide_asan.cpp
tests/sanitize/scale_asan: tests/sanitize/scale_asan.cpp $(CSRC)/hl_scale.h $(CSRC)/hl_ingest.h
	$(HIPCC) $(SANFLAGS) $(ASAN) $(UBSAN) -o $@ -x c++ tests/sanitize/scale_asan.cpp
tests/sanitize/ladder_asan: tests/sanitize/ladder_asan.cpp $(CSRC)/hl_ladder.h $(CSRC)/hl_scale.h $(CSRC)/hl_ingest.h
	$(HIPCC) $(SANFLAGS) $(ASAN) $(UBSAN) -o $@ -x c++ tests/sanitize/ladder_asan.cpp
# the emulator under UndefinedBehaviorSanitizer too: a 16-minute compile of
# the kernel logic, run once per change of the shift / overflow idioms
# (DESIGN.md §2); tests/test_sanitizers.py uses it when it is present
ubsan: tests/sanitize/libhl_emu_ubsan.so
tests/sanitize/libhl_emu_ubsan.so: $(EMUSRC) $(EMUINC) $(HOSTSRC) $(HDRS)
	$(HIPCC) --offload-arch=$(ARCH) $(SANFLAGS) -DHL_FAM3=1 $(ASAN) $(UBSAN) -shared-libsan -shared -o $@ $(EMUSRC) $(HOSTSRC)

# profiling build: same library (same device scheduling flags) with per-phase
# clock64 counters (tools/phase_profile.py)
profile: build/prof/hartallo_amd/libhartallo_amd.so
build/prof/hartallo_amd/libhartallo_amd.so: $(KSRC) $(HOSTSRC) $(HDRS) $(INGOBJ)
	mkdir -p build/prof/hartallo_amd
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) $(DEVFLAGS) -DHL_PROFILE=1 -shared -o $@ $(KSRC) $(HOSTSRC) -x none $(INGOBJ)

# debug builds: LDS poisoned before every macroblock with two different salts
# (tools/gpu_diag.sh); any output difference names a read of uninitialised LDS
poison: build/poison1/libhartallo_amd.so build/poison2/libhartallo_amd.so
build/poison%/libhartallo_amd.so: $(KSRC) $(HOSTSRC) $(HDRS) $(INGOBJ)
	mkdir -p build/poison$*
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) $(DEVFLAGS) -DHL_POISON_LDS=$* -shared -o $@ $(KSRC) $(HOSTSRC) -x none $(INGOBJ)

# memory-scope variants of the pipelined run's fences (diagnostics)
scopes: build/acqsys/libhartallo_amd.so build/relacqsys/libhartallo_amd.so
build/acqsys/libhartallo_amd.so: $(KSRC) $(HOSTSRC) $(HDRS) $(INGOBJ)
	mkdir -p build/acqsys
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) $(DEVFLAGS) '-DHL_ACQ_SCOPE=""' -shared -o $@ $(KSRC) $(HOSTSRC) -x none $(INGOBJ)
build/relacqsys/libhartallo_amd.so: $(KSRC) $(HOSTSRC) $(HDRS) $(INGOBJ)
	mkdir -p build/relacqsys
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) $(DEVFLAGS) '-DHL_ACQ_SCOPE=""' '-DHL_REL_SCOPE=""' -shared -o $@ $(KSRC) $(HOSTSRC) -x none $(INGOBJ)

# variants of the product for A/B runs: make variant V=<name> VDEFS="-D..."
variant: build/$(V)/libhartallo_amd.so
build/$(V)/libhartallo_amd.so: $(KSRC) $(HOSTSRC) $(HDRS) $(INGOBJ)
	mkdir -p build/$(V)
	$(HIPCC) --offload-arch=$(ARCH) $(CXXFLAGS) $(DEVFLAGS) $(VDEFS) -shared -o $@ $(KSRC) $(HOSTSRC) -x none $(INGOBJ)

# (then the drivers with a per-frame schedule, tests/refdrive, where the reference library was built)
oracle: product  # oracle/_ref/drop_in_enc links the product library
	$(MAKE) -C oracle
	if [ -f oracle/_ref/libhl.a ] && [ -d $(REF)/source ]; then $(MAKE) -C tests/refdrive REF=$(REF); fi

clean:
	rm -f $(INGOBJ) tests/emu/libhl_scale_emu.so tests/emu/libhl_ladder_emu.so tests/sanitize/scale_asan tests/sanitize/ladder_asan hartallo_amd/libhartallo_amd.so tests/emu/libhl_emu.so tests/emu/libhl_pyr_emu.so tests/emu/libhl_scene_emu.so tests/emu/libhl_quality_emu.so tests/emu/libhl_ingest_emu.so tests/emu/libhl_display_emu.so tests/emu/libhl_svc_display_emu.so tests/emu/libhl_svc_geom_emu.so tests/emu/libhl_rec_emu.so tests/emu/libhl_sched_emu.so tests/gpu_unit/libhl_unit.so tests/gpu_unit/libhl_unit_cand.so tests/gpu_unit/libhl_unit_rec.so tests/sanitize/*.so tests/sanitize/*.o tests/sanitize/rowgate_tsan tests/sanitize/pop_tsan tests/sanitize/ingest_asan tests/sanitize/ingest_edge_asan tests/sanitize/ingest_wide_asan
	$(MAKE) -C oracle clean
