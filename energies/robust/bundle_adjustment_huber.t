-- Bundle adjustment with a Huber loss on the reprojection error: bundle_adjustment.t with
-- the block preconditioner and its two reprojection rows in one RobustEnergy statement.
-- Each observation is one loss block, s = |projection - measurement|^2, and contributes
-- 1/2 rho(s), rho(s) = s up to s = a^2 and 2 a sqrt(s) - a^2 beyond: a mismatched observation
-- pulls with a bounded force (INTEGRATION.md, Robust losses). The scale a is the Param
-- "huber", one more entry at the end of problemparams; it is re-read whenever the weights
-- are evaluated, so a caller may anneal it between Steps.
local NC, NP, NO = Dim("NC", 0), Dim("NP", 1), Dim("NO", 2)

local w_cam = Param("w_cam", float, 0)
local w_pt  = Param("w_pt", float, 1)
local CamR  = Unknown("CamR", opt_float3, {NC}, 2)   -- Euler angles
local CamT  = Unknown("CamT", opt_float3, {NC}, 3)
local X     = Unknown("X", opt_float3, {NP}, 4)
local CamR0 = Array("CamR0", opt_float3, {NC}, 5)
local CamT0 = Array("CamT0", opt_float3, {NC}, 6)
local X0    = Array("X0", opt_float3, {NP}, 7)
local Obs   = Array("Obs", opt_float2, {NO}, 8)      -- measured image positions
local huber = Param("huber", float, 12)
local G     = Graph("G", {NO}, "c", {NC}, 9, "p", {NP}, 10, "o", {NO}, 11)
UsePreconditioner("block")

Energy(w_cam * (CamR(0) - CamR0(0)))
Energy(w_cam * (CamT(0) - CamT0(0)))
Energy(w_pt * (X(0) - X0(0)))

local q = Rotate3D(CamR(G.c), X(G.p)) + CamT(G.c)
local m = Obs(G.o)
RobustEnergy("huber", huber, q(0) / q(2) - m(0), q(1) / q(2) - m(1))
