-- An image with a per-row bias: two unknowns over different index spaces.
-- I ({W,H}) is a smooth image and B ({H}) one offset per row (a line-scan sensor's row
-- gain drift); each measured pixel (an edge of the graph, {E}) says I + B of its row equals
-- the data D there. Pixels with Mask = 1 are held fixed (Exclude applies to the image's
-- space; every B stays active). Runs on generated kernels.
local W, H, E = Dim("W", 0), Dim("H", 1), Dim("E", 2)

local w_s  = Param("w_s", float, 0)
local w_b  = Param("w_b", float, 1)
local I    = Unknown("I", opt_float, {W, H}, 2)
local B    = Unknown("B", opt_float, {H}, 3)
local D    = Array("D", opt_float, {W, H}, 4)
local Mask = Array("Mask", opt_float, {W, H}, 5)
local G    = Graph("G", {E}, "px", {W, H}, 6, "row", {H}, 7)

Exclude(eq(Mask(0, 0), 1))

Energy(I(G.px) + B(G.row) - D(G.px))
Energy(Select(InBounds(1, 0), w_s * (I(0, 0) - I(1, 0)), 0))
Energy(Select(InBounds(0, 1), w_s * (I(0, 0) - I(0, 1)), 0))
Energy(w_b * B(0))
