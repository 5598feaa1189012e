# Build lib/libdiffattn_<name>.so beside the regular library: the csrc Makefile with its own
# object directory (csrc/build_v/<name>) and the extra flags on the named units (the
# Makefile's EXTRA_<unit> hook), so the link list is always the Makefile's SRCS.
#   bash tools/build_variant.sh <name> <unit>[,<unit>...] "<flags>"
#   bash tools/build_variant.sh stamps attn_bf16 "-DDTA_STAMPS=1"
#   bash tools/build_variant.sh c512 capi,decode "-DDTA_DECODE_CHUNK=512"
# Load the result with DTA_LIB=<path> or as name=lib/libdiffattn_<name>.so (tools/ab_kernels.py).
set -e
NAME=$1; UNITS=$2; EXTRA=$3
[ -n "$NAME" ] && [ -n "$UNITS" ] || { echo "usage: $0 <name> <unit>[,<unit>...] \"<flags>\"" >&2; exit 2; }
C=$(dirname $0)/../differential_transformer_replication_amd/csrc
ARGS=()
for u in ${UNITS//,/ }; do
  [ -f $C/$u.hip ] || { echo "no unit $u.hip in $C" >&2; exit 2; }
  ARGS+=("EXTRA_$u=$EXTRA")
done
make -C $C -j${JOBS:-8} BUILD=build_v/$NAME OUT=../lib/libdiffattn_$NAME.so "${ARGS[@]}"
echo built lib/libdiffattn_$NAME.so
