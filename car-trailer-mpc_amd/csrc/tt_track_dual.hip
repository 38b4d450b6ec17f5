// The tracking kernels once more, with the multiplier export (TrackArgs::dual) in their epilogue: launch_track_dual.
// A translation unit of its own so that the plain kernels' code object stays what it is without the export (see the
// head of tt_track.hip).
#define TT_TRACK_DUAL 1
#include "tt_track.hip"
