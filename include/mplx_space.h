/* mplx_space.h -- part of the C-ABI of libmplx.so: included by mplx.h (include that one), inside its extern "C" block and after its
 * declarations of mplx_ctx and mplx_cloud.  mpl_ros_amd/_capi.py lists these entry points in EXPORTS_SPACE. */
#ifndef MPLX_SPACE_H
#define MPLX_SPACE_H

/* The state spaces of a LIST OF QUERIES of the context's last mplx_plan / mplx_plan_batch / mplx_plan_batch_wait, exported by kernels
 * straight from the device pools, one launch per pass for the whole list: the states with g, h and the closed / opened flags
 * (getCloseSet / getOpenSet) and the predecessor records behind getValidPrimitives / getAllPrimitives.
 *   qs        n_q distinct query indices of the last batch; NULL: the queries 0 .. n_q - 1.  One query is a list of one.
 *   outputs   concatenated in the order of qs; NULL arrays are allowed (only what is asked for crosses the bus).  A query that
 *             created no state (occupied start, start inside the goal tolerance) contributes zero rows, whatever its status.
 *   _counts   host only, launches nothing: node_off / edge_off hold n_q + 1 entries, query qs[i] owns the rows
 *             [node_off[i], node_off[i + 1]) of the per-state arrays and [edge_off[i], edge_off[i + 1]) of the per-record arrays.
 *   _space    states: 14 doubles per row -- pos3 vel3 acc3 jrk3 yaw t; derivatives the control kind does not carry are 0, yaw is 0
 *             unless the search carried it (MPLX_YAW).  cap_nodes: rows the arrays hold.
 *   _edges    one record per predecessor entry: for every state in id order its entries oldest first (the order the reference's
 *             pred vectors grow in); child / parent are the query's OWN node ids (not offset by the concatenation), action the
 *             control input.  cap_edges: rows the arrays hold.
 *   _ms       (measurement) kernel time of the last nodes + scan pass and of the last edges pass that ran.  Passes already done for
 *             the same (plan, query list) are not repeated; a states-only caller never runs the edges pass.
 * MPLX_ERR_CAPACITY, nothing written: the arrays are too small.  MPLX_ERR_ARG, nothing written, nothing launched, text in
 * mplx_last_error: a null handle; no batch, or the last launch was aborted; a submitted batch still outstanding; pools released
 * (mplx_release_pools); a batch that ran with pool recycling; n_q <= 0, a duplicate or a q outside the batch; a listed query that
 * created states and ended MPLX_PLAN_POOL_FULL or MPLX_PLAN_INTERNAL (its last records may be half built; the text names it) -- or with
 * any other status than MPLX_PLAN_OK / _NO_PATH / _MAX_EXPAND / _TRAJ_TOO_LONG, such as a query ended by the launch guard: only
 * those four are known to leave a consistent state space; and, after the first pass, predecessor lists that do not hold exactly
 * the records the search counted ("corrupt predecessor list").
 * (mplx_result_nodes / _edges / _blocked and mplx_debug_query_records of mplx.h are the host-decoded getters; they stay.) */
int mplx_result_space_counts(mplx_ctx *ctx, int32_t n_q, const int32_t *qs, uint64_t *node_off /* n_q + 1 */, uint64_t *edge_off /* n_q + 1 */);
int mplx_result_space(mplx_ctx *ctx, int32_t n_q, const int32_t *qs, uint64_t cap_nodes, double *states /* rows x 14 */, double *g, double *h,
                      int32_t *closed, int32_t *opened);
int mplx_result_space_edges(mplx_ctx *ctx, int32_t n_q, const int32_t *qs, uint64_t cap_edges, int32_t *child, int32_t *parent, int32_t *action);
int mplx_result_space_ms(const mplx_ctx *ctx, float ms[2]);

/* The same for the queries of the last mplx_cloud_plan_batch, on the point-cloud planner's internal context: 13 doubles per row --
 * pos3 vel3 acc3 jrk3 t, as mplx_cloud_result_nodes decodes them -- and the text of a refusal in mplx_cloud_last_error.  (env_cloud
 * skips blocked primitives: every record is a valid primitive.) */
int mplx_cloud_result_space_counts(mplx_cloud *c, int32_t n_q, const int32_t *qs, uint64_t *node_off /* n_q + 1 */, uint64_t *edge_off /* n_q + 1 */);
int mplx_cloud_result_space(mplx_cloud *c, int32_t n_q, const int32_t *qs, uint64_t cap_nodes, double *states /* rows x 13 */, double *g, double *h,
                            int32_t *closed, int32_t *opened);
int mplx_cloud_result_space_edges(mplx_cloud *c, int32_t n_q, const int32_t *qs, uint64_t cap_edges, int32_t *child, int32_t *parent, int32_t *action);
int mplx_cloud_result_space_ms(const mplx_cloud *c, float ms[2]);

#endif
