#!/bin/bash
# AddressSanitizer + UBSan run of the HOST code the two batch provers share (csrc/pbs_prove_pool.hip, their two owners, vpbs::key_hash_links
# in api.hip and its caller in verify_pbs_batch.hip) through a stand-alone program, tools/asan_pool_host.hip: no device, no Python, no
# preloaded runtime.  Those five files are instrumented on the host side only (device code is compiled without sanitizer); the rest of the
# library is linked from the product build's objects, so build the library first (make -C verifiable-fhe-paper_amd/csrc).
set -e
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT=/tmp/vpbs_asan_pool; mkdir -p $OUT; rm -f $OUT/*.o
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
INSTRUMENTED="api pbs_prove_pool pbs_prove_batch pbs_prove_ring verify_pbs_batch"
pids=""
cd "$ROOT/verifiable-fhe-paper_amd/csrc"
for f in $INSTRUMENTED; do
  /opt/rocm/bin/hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 $SAN -Wno-unused-function -Wno-pass-failed -c $f.hip -o $OUT/$f.o &
  pids="$pids $!"
done
for p in $pids; do wait $p; done   # a failed compile ends the run
REST=""
for o in _build/*.o; do
  case " $INSTRUMENTED " in *" $(basename $o .o) "*) ;; *) REST="$REST $o" ;; esac
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $SAN -o $OUT/libvpbs_hip.so $OUT/*.o $REST
/opt/rocm/bin/hipcc -O1 -g -std=c++17 --offload-arch=gfx950 $SAN "$ROOT/tools/asan_pool_host.hip" -o $OUT/asan_pool_host \
  -L$OUT -lvpbs_hip -Wl,-rpath,$OUT
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 $OUT/asan_pool_host
