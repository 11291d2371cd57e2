/* mplx_poly3_space.h -- part of the C-ABI of libmplx.so: included by mplx.h (include that one), inside its extern "C" block and
 * after its declaration of mplx_poly3.  mpl_ros_amd/_capi.py lists these entry points in EXPORTS_POLY3_SPACE. */
#ifndef MPLX_POLY3_SPACE_H
#define MPLX_POLY3_SPACE_H

/* The state space of query q of the last mplx_poly3_plan_batch, exported by kernels straight from the device pools: mplx_poly_result_nodes
 * / _edges / _blocked / _space_ms and mplx_poly_plan_epoch word for word, with 13-column states (pos3 vel3 acc3 jrk3 t: acc is 0 under
 * ACC, jrk always).  Served after MPLX_PLAN_OK / _NO_PATH / _MAX_EXPAND / _TRAJ_TOO_LONG; a query that created no state gives MPLX_OK,
 * nothing written, *n = 0; _space with cap < n_nodes: MPLX_ERR_CAPACITY, nothing written; _edges / _blocked: *n is always the full count,
 * at most cap entries are written.  Refused (MPLX_ERR_ARG, text in mplx_poly3_last_error): MPLX_PLAN_POOL_FULL / _INTERNAL queries, q
 * outside the last batch, released pools, a null handle, and for _blocked mplx_poly3_config or mplx_poly3_commit since the plan.
 * (mplx_poly3_result_nodes of mplx.h is the host-decoded getter of positions and flags; this is the export with h and the records.) */
int mplx_poly3_result_space(mplx_poly3 *p, int32_t q, uint64_t cap, double *states /* n x 13 */, double *g, double *h, int32_t *closed, int32_t *opened);
int mplx_poly3_result_edges(mplx_poly3 *p, int32_t q, uint64_t cap, int32_t *child, int32_t *parent, int32_t *action, uint64_t *n);
int mplx_poly3_result_blocked(mplx_poly3 *p, int32_t q, uint64_t cap, int32_t *parent, int32_t *action, uint64_t *n);
int mplx_poly3_result_space_ms(mplx_poly3 *p, float ms[3]);
uint64_t mplx_poly3_plan_epoch(const mplx_poly3 *p);

#endif
