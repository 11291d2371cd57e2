// mplx_plpa_space.h -- (internal) the scratch buffers of a handle's state-space exports (mplx_plpa_export_* / mplx_plpa3_export_*,
// mplx_plpa_space.hip): owned by the mplx_plpa / mplx_plpa3 handle, created by its first export, released with the handle.
#pragma once

struct mplx_plpa_space;
void mplx_plpa_space_free(mplx_plpa_space *s);  // (null: nothing to do)
