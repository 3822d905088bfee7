# Where the attention kernel's time goes: what-if builds (timing aids, wrong results) next to the product library.
# All six macros act on the four-wave kernel (attention2q_kernel): NOBIAS / NOEXP / NOS / NOPV change the shared f16x2 flash step
# (Att2Wave in csrc/attention.hip, both QB instances), NOSTAGE and -DKN_ATT_PROF (in-kernel cycle counters) its schedule.  The
# eight-wave kernel that the default shape 21 x 1500 x 16 dispatches (attention2w_kernel) has none of them, so every run here
# sets KNNSVC_ATT_NW=4.
#   cd knn_svc_amd/csrc && for v in NOBIAS NOEXP NOS NOPV NOSTAGE; do make BUILD=build_att_$v OUT=../libknnsvc_att_$v.so EXTRA=-DKN_ATT_$v; done
cd $GRAFT_REPO_ROOT
export KNNSVC_ATT_NW=4
echo "product:"; python tools/attn_bench.py 2>&1 | grep "pre-split"
for v in NOBIAS NOEXP NOS NOPV NOSTAGE; do
  echo "$v:"; KNNSVC_LIB=$GRAFT_REPO_ROOT/knn_svc_amd/libknnsvc_att_$v.so python tools/attn_bench.py 2>&1 | grep "pre-split"
done
