-- Bundle adjustment with the points eliminated, the reduced camera system formed explicitly
-- and solved directly: bundle_adjustment_schur_explicit.t plus LinearSolver("cholesky"). Each
-- Step fills S (+ LM's diagonal) into dense tiles, factors it S = L L^T and takes the exact
-- Gauss-Newton / LM step instead of lIterations of PCG (lIterations > 0 only switches the
-- linear solve on). Same problemparams, same energy. Runs on generated kernels.
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
local G     = Graph("G", {NO}, "c", {NC}, 9, "p", {NP}, 10, "o", {NO}, 11)
UsePreconditioner(true)
Eliminate(X)
ReducedSystem("explicit")
LinearSolver("cholesky")

Energy(w_cam * (CamR(0) - CamR0(0)))
Energy(w_cam * (CamT(0) - CamT0(0)))
Energy(w_pt * (X(0) - X0(0)))

local q = Rotate3D(CamR(G.c), X(G.p)) + CamT(G.c)
local m = Obs(G.o)
Energy(q(0) / q(2) - m(0))
Energy(q(1) / q(2) - m(1))
