------------------------------ MODULE ac_error ------------------------------
(* An evaluation error INSIDE an action constraint (a division by zero on the first step) is reported as TLC reports one inside an invariant. *)
EXTENDS Naturals, Sequences, TLC

(* --algorithm ac_error
variables x = 0;

process P = 1
begin
  a: x := 1;
  b: x := 2;
end process

end algorithm *)

Ratio == x' \div x >= 0
=============================================================================
