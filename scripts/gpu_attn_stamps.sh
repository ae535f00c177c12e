# Stage stamps of the decode attention (scripts/attn_stamps.hip -> profiles/attn_ramp/README.md).  Build first, where hipcc is:
#   mkdir -p build && hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -Imoshi_amd/csrc scripts/attn_stamps.hip moshi_amd/csrc/api_common.hip -o build/attn_stamps
# then, on the MI355X, this script: one GPU step, run once.
cd "$(dirname "$0")/.." || exit 1
timeout -k 10 120 build/attn_stamps > build/attn_stamps.txt 2>&1
rc=$?
grep "^depth" build/attn_stamps.txt
exit $rc
