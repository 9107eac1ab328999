#!/bin/bash
# Builds hostcxx/_build/muscle_gpu: the reference's own `muscle` with the MI355X posterior stage
# linked in as a drop-in. Needs the reference objects that oracle/build_ref.sh
# compiles from the sources where they lie ($MUSCLE_REF_SRC, default /root/reference/src) — nothing
# of the reference is copied into the repo, and the combined (GPL-3.0) binary is git-ignored. A copy
# is kept beside the compiled reference as oracle/_ref/muscle_gpu, which travels with it to a GPU
# box: where the reference sources are absent, this script installs that copy instead of linking.
# The copy is also kept under a name that carries a digest of the drop-in's sources (oracle/_ref/muscle_gpu.<digest>): an
# oracle/_ref that serves several checkouts (two commits built one after the other) holds a binary for each, and a checkout
# without the reference sources installs the one linked from ITS hostcxx/ — the plain name only when there is none, with a warning.
#
#   reference objects  - consflat.o, alnalnsflat.o, alnmsasflat.o, buildpostflat.o, alignpairflat.o, refineflat.o  (MPCFlat::ConsIter,
#                        MPCFlat::AlignAlns, PProg::AlignMSAsFlat, MPCFlat::BuildPost, AlignPairFlat(_SparsePost) and
#                        MPCFlat::RefineIter — each alone in its translation unit in the reference — are ours)
#                      - calcposteriorflat.o's CalcPosterior symbol, weakened with objcopy so that
#                        hostcxx/mpcflat_gpu.cpp's strong definition wins while CalcPostFlat and the
#                        two vestigial virtuals in the same object stay available; likewise one member each of
#                        super7.o, uclust.o, pprog2.o, mpcflat.o (MPCFlat::CalcPosteriors), swdistmx.o (CalcGuideTree_SW_BLOSUM62) and
#                        eadistmx.o (CalcEADistMx) - see below
#   + hostcxx/mpcflat_gpu.cpp (g++, against the reference headers) + hostcxx/rand_isolate.cpp
#     (-Wl,--wrap=rand) + -lmpcgpu
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(dirname "$HERE")"
SRC="${MUSCLE_REF_SRC:-/root/reference/src}"
REFOBJ="$ROOT/oracle/_ref/obj"
OUT="$HERE/_build"
PREBUILT="$ROOT/oracle/_ref/muscle_gpu"
DIGEST=$(cat "$HERE/mpcflat_gpu.cpp" "$HERE/rand_isolate.cpp" "$HERE/build_muscle_gpu.sh" "$ROOT/include/mpcgpu.h" | sha256sum | cut -c1-16)
if [ ! -d "$SRC" ] || [ ! -d "$REFOBJ" ]; then
  if [ -z "${MPCGPU_BIN:-}" ] && [ -x "$PREBUILT.$DIGEST" ]; then
    mkdir -p "$OUT"
    cp -p "$PREBUILT.$DIGEST" "$OUT/muscle_gpu"
    echo "installed: $OUT/muscle_gpu (from $PREBUILT.$DIGEST; the reference sources are not here)"
    exit 0
  fi
  if [ -z "${MPCGPU_BIN:-}" ] && [ -x "$PREBUILT" ]; then
    mkdir -p "$OUT"
    cp -p "$PREBUILT" "$OUT/muscle_gpu"
    echo "installed: $OUT/muscle_gpu (from $PREBUILT; the reference sources are not here)"
    echo "build_muscle_gpu.sh: WARNING: no $PREBUILT.$DIGEST - the installed binary may have been linked from other drop-in sources than this tree's hostcxx/" >&2
    exit 0
  fi
  echo "build_muscle_gpu.sh: reference sources/objects not available (run oracle/build_ref.sh where the reference sources are) - skipping" >&2
  exit 0
fi
mkdir -p "$OUT"
CXXFLAGS="-std=c++17 -O3 -fopenmp -DNDEBUG -pthread -fPIC -w -I$ROOT/oracle/_ref/inc -I$SRC -I$ROOT/include"
g++ $CXXFLAGS -c "$HERE/mpcflat_gpu.cpp" -o "$OUT/mpcflat_gpu.o"
g++ $CXXFLAGS -c "$HERE/rand_isolate.cpp" -o "$OUT/rand_isolate.o"
objcopy --weaken-symbol=_ZN7MPCFlat13CalcPosteriorEj "$REFOBJ/calcposteriorflat.o" "$OUT/calcposteriorflat_weak.o"
# MPCFlat::BuildPost is ours too (hostcxx/mpcflat_gpu.cpp -> mpcgpu_build_post): buildpostflat.o is not linked at all
rm -f "$OUT/buildpostflat_ref.o"
# Super7::IntraAlignShrubs: ours (parallel over device contexts); the rest of super7.o stays
objcopy --weaken-symbol=_ZN6Super716IntraAlignShrubsEv "$REFOBJ/super7.o" "$OUT/super7_weak.o"
# UClust::Search: ours (all word-count hits aligned in one library call); AlignPairFlat / AlignPairFlat_SparsePost: ours
# (alignpairflat.o is not linked)
# UClust::Run: ours too (the loop by windows, one mpcgpu_search_pairs call per window); the reference's body stays reachable under a
# second, global name at the same address, UClust_Run_ref (MUSCLE_GPU_UCLUST_WINDOW=0 and unset call it)
UCSYM=_ZN6UClust3RunER13MultiSequencef
read -r UCVAL UCSEC < <(objdump -t "$REFOBJ/uclust.o" | awk -v s="$UCSYM" '$NF == s && $2 == "g" { print $1, $4 }')
objcopy --weaken-symbol=_ZN6UClust6SearchEjRNSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEE --weaken-symbol="$UCSYM" \
  --add-symbol "UClust_Run_ref=$UCSEC:0x$UCVAL,global,function" "$REFOBJ/uclust.o" "$OUT/uclust_weak.o"
# PProg::Run2: ours (independent joins of the guide tree side by side); AlignAndJoin and the rest of pprog2.o stay
objcopy --weaken-symbol=_ZN5PProg4Run2ERKSt6vectorIjSaIjEES4_ "$REFOBJ/pprog2.o" "$OUT/pprog2_weak.o"
# MPCFlat::CalcPosteriors: ours (a plain loop: the work of all pairs happens inside the first CalcPosterior call); the rest of mpcflat.o stays
objcopy --weaken-symbol=_ZN7MPCFlat14CalcPosteriorsEv "$REFOBJ/mpcflat.o" "$OUT/mpcflat_weak.o"
# MPCFlat::ProgressiveAlign: ours (the joins of a guide-tree level in one library call); the reference's stays in the binary as
# MPCFlat_ProgressiveAlign_ref (our fallback calls it); ProgAln, FreeProgMSAs, FreeSparsePosts of progalnflat.o stay as they are
objcopy --redefine-sym _ZN7MPCFlat16ProgressiveAlignEv=MPCFlat_ProgressiveAlign_ref "$REFOBJ/progalnflat.o" "$OUT/progalnflat_weak.o"
# CalcGuideTree_SW_BLOSUM62: ours (all-pairs Smith-Waterman scores from the device: the guide tree of -super7 / -super7_mega / -swdistmx
# without a tree option). The symbol is weakened in swdistmx.o, so cmd_swdistmx in the same object reaches our definition like
# cmd_super7 and cmd_super7_mega do; the reference's function stays reachable under a second, global name at the same address,
# CalcGuideTree_SW_BLOSUM62_ref (MUSCLE_GPU_SW_TREE=0 calls it).
SWSYM=_Z25CalcGuideTree_SW_BLOSUM62RK13MultiSequenceR4Tree
read -r SWVAL SWSEC < <(objdump -t "$REFOBJ/swdistmx.o" | awk -v s="$SWSYM" '$NF == s && $2 == "g" { print $1, $4 }')
objcopy --weaken-symbol="$SWSYM" --add-symbol "CalcGuideTree_SW_BLOSUM62_ref=$SWSEC:0x$SWVAL,global,function" "$REFOBJ/swdistmx.o" "$OUT/swdistmx_weak.o"
# CalcEADistMx: ours (the EA of all pairs in one library call: `-eadistmx`, and the guide tree over the consensus sequences of -super4 /
# -super5 through Super4::CalcConsensusSeqsDistMx). Handled like the function above: weakened in eadistmx.o, so cmd_eadistmx in the same
# object — which stays the reference's — reaches our definition; the reference's loop stays reachable as CalcEADistMx_ref (a caller that
# wants the sparse posteriors, and MUSCLE_GPU_EA_DISTMX=0).
EASYM=$(objdump -t "$REFOBJ/eadistmx.o" | awk '$2 == "g" && $NF ~ /^_Z12CalcEADistMxP/ { print $NF }')
read -r EAVAL EASEC < <(objdump -t "$REFOBJ/eadistmx.o" | awk -v s="$EASYM" '$NF == s && $2 == "g" { print $1, $4 }')
objcopy --weaken-symbol="$EASYM" --add-symbol "CalcEADistMx_ref=$EASEC:0x$EAVAL,global,function" "$REFOBJ/eadistmx.o" "$OUT/eadistmx_weak.o"
OBJS=$(ls "$REFOBJ"/*.o | grep -v -e '/super7\.o$' -e '/uclust\.o$' -e '/alignpairflat\.o$' -e '/pprog2\.o$' -e '/mpcflat\.o$' -e '/progalnflat\.o$' -e '/swdistmx\.o$' -e '/eadistmx\.o$' | grep -v -e '/consflat\.o$' -e '/alnalnsflat\.o$' -e '/alnmsasflat\.o$' -e '/calcposteriorflat\.o$' -e '/buildpostflat\.o$' -e '/refineflat\.o$')
# The product links libmpcgpu.so. tests/test_dropin_emu.py re-runs this script with
# MPCGPU_LIBDIR/MPCGPU_LIBNAME pointing at the SIMT-emulator build of the same library sources
# (tests/emu, test infrastructure) to check the host-side plumbing of this file without a GPU.
LIBDIR="${MPCGPU_LIBDIR:-$ROOT/muscle_amd/csrc}"
LIBNAME="${MPCGPU_LIBNAME:-mpcgpu}"
BIN="${MPCGPU_BIN:-muscle_gpu}"
# --wrap=rand: the reference's rand() (refineflat.cpp:14) gets a private copy of glibc's default
# stream; the HIP runtime in the same process otherwise consumes it (hostcxx/rand_isolate.cpp)
g++ -O3 -fopenmp -pthread -Wl,--wrap=rand $OBJS "$OUT/calcposteriorflat_weak.o" "$OUT/super7_weak.o" "$OUT/uclust_weak.o" "$OUT/pprog2_weak.o" "$OUT/mpcflat_weak.o" "$OUT/progalnflat_weak.o" "$OUT/swdistmx_weak.o" "$OUT/eadistmx_weak.o" "$OUT/mpcflat_gpu.o" "$OUT/rand_isolate.o" \
  -L"$LIBDIR" -l"$LIBNAME" -Wl,-rpath,'$ORIGIN/../../muscle_amd/csrc' -Wl,-rpath,"$LIBDIR" -Wl,-rpath,/opt/rocm/lib -o "$OUT/$BIN"
echo "built: $OUT/$BIN"
# the product binary, beside the compiled reference (same depth below the root: the $ORIGIN run path holds from there too)
if [ -z "${MPCGPU_BIN:-}" ]; then
  cp -p "$OUT/$BIN" "$PREBUILT"
  cp -p "$OUT/$BIN" "$PREBUILT.$DIGEST"
fi
